"""CPU check of msj_select_elements_device's arithmetic (mojo_simdjson_amd/csrc/select_elements_math.h).

The definition in include/msj_stage1.h is restated in Python from its text alone (`definition` below): per document the
value tests/select_reference.py finds for the list's path; a list gives one row per item, and each pointer is looked up in
the item by the same reference (an item that is no object gives 17 for any pointer but ""; the first of duplicate keys
wins).  The host twin (tests/select_elements_math_host.cpp: the verdict on the rows, the order test, the row states and the
member test of the header with select_math.h's compare and record, serially) runs over the element records of the
array-column twin (tests/test_array_column_math.py); every record decoded back to a Python value must equal the
definition's, fill and canary behind the records included.  Hostile records -- which json cannot describe -- are pinned by
value.  The kernels that run the same header on the device are covered by tests/test_select_elements.py (-m gpu).
"""
import ctypes
import json
import os
import random
import subprocess

import numpy as np
import pytest

from mojo_simdjson_amd import _lib
from mojo_simdjson_amd.document_stream import FIELD_DTYPE, field_value
from tests import helpers
from tests import select_reference as ref
from tests import test_array_column_math as tac
from tests import test_number_math as tnm
from tests import test_select_math as tsm
from tests import test_tape_documents_math as tdk
from tests import test_validate_documents_math as tdm
from tests import test_validate_math as tvm

MSJ_CAPACITY, BAD_ARGUMENT = 1, -1
NO_TOKEN = 0xFFFFFFFF

# the list at /items (or, for a document that is an array, at ""), and what is looked up in its elements
PINS = [b'{"items":[{"sku":"a","qty":2},{"qty":3},7,"s",[],{},null]}',
        b'{"items":[{"x":{"sku":1},"sku":2}]}',                       # the depth test: a deeper key must not match
        b'{"items":[{"a":[{"sku":9}]},{"sku":1}]}',                   # ... nor one of an object in a nested array
        b'{"items":[{"sku":1,"sku":2},{"sku":3},{"sku":4,"qty":[]}]}',    # duplicates inside one element; the same key in neighbours
        b'{"items":[{"s\\u006bu":"e\\nv\\u00e9","qty":1.5}]}',      # an escaped key, an escaped value
        b'{"items":[{"dims":{"w":1}},{"qty":1},{"dims":5},{"dims":{"h":2}},{"dims":{"w":{"w":3}},"w":7}]}',
        b'{"items":[]}', b'{"other":[{"sku":1}]}', b'{"items":7}', b'{"items":{"sku":1}}',
        b'{"items":[{"sku":-12,"qty":1e2},{"sku":9223372036854775807}]}',
        b'{"x":[{"sku":5}],"items":[{"":0,"sku":{}}]}']
ROOT_PINS = [b'[{"x":{"sku":1},"sku":2}]', b'[{"a":[{"sku":9}]},{"sku":1}]', b"[]", b'{"sku":1}', b'[[{"sku":1}],{"sku":[2]}]', b"7"]
PIN_PATHS = ["/sku", "/qty", "/dims/w", "", "/dims", "/a", "/", "/dims/w/w"]
SIXTEEN = ["/sku", "/qty", "/dims", "/dims/w", "/dims/h", "", "/a", "/x", "/x/sku", "/w", "/", "/sk", "/skuu", "/s~0ku", "/dims/w/w", "/other"]

_twin = None


def load_twin():
    """The host twin of the call (g++ build of tests/select_elements_math_host.cpp)."""
    global _twin
    if _twin is not None:
        return _twin
    os.makedirs(tvm.BUILD, exist_ok=True)
    so = os.path.join(tvm.BUILD, "libselect_elements_math_host.so")
    src = os.path.join(helpers.ROOT, "tests", "select_elements_math_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    for name, args, res in (("sem_select_elements", [vp, ctypes.c_char_p, u64, vp, u64] + [vp] * 6 + [u64, vp, vp, vp, vp, u64, vp], None),
                            ("sem_rows_below", [vp, u32, u32], u32), ("sem_state_rows", [u64, u64], u64),
                            ("sem_row_state", [u32, u32, u32, u32, u64, vp, vp], u32)):
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
def twins():
    return Twins()


class Twins:
    """The verdict, select, array-column and element-select twins"""

    def __init__(self):
        self.v, self.s, self.a, self.e = tdm.load_twin(), tsm.load_twin(), tac.load_twin(), load_twin()


# ---- the twin ---------------------------------------------------------------------------------------------------------------

def element_rows(twins, w, list_pointer, verdicts=None, elements_capacity=None):
    """The element records of one path's arrays, as the select twin and the array-column twin give them
    -> (tac.Lists, records FIELD_DTYPE[n_elements written], its msj_select_documents_result)"""
    column = tsm.twin_select(twins.s, w, [list_pointer], verdicts=verdicts).column(0)[:w.D].copy()
    lists = tac.twin_lists(twins.a, w, column, elements_capacity=elements_capacity)
    n = min(int(lists.res.n_elements), lists.elements_capacity)
    return lists, lists.elements[:n].copy(), lists.esel


def rows_result(R, code=0):
    return _lib.MsjSelectDocumentsResult(code, 0, R, 1, R, 0, 0)


def twin_elements(twins, w, pointers, rows, rows_select=None, capacity=None, numbers=True, numbers_result=True, numbers_capacity=None):
    """sem_select_elements over the window's arrays and the records `rows`.  rows_select None: a result for len(rows) rows.
    numbers False: d_numbers NULL with capacity 0; numbers_result False: d_numbers_result NULL.  -> tsm.Selected"""
    rc, blob, _ = tsm.compile_paths(twins.s, pointers)
    assert rc == 0, (rc, pointers)
    rows = np.ascontiguousarray(rows)
    rows_select = rows_result(rows.size) if rows_select is None else rows_select
    capacity = max(rows.size, 1) if capacity is None else capacity
    fields = tsm.filled_fields(len(pointers), capacity)
    res = _lib.MsjSelectDocumentsResult()
    ncap = (int(w.records.size) if numbers_capacity is None else numbers_capacity) if numbers else 0
    recs = np.ascontiguousarray(w.records[:ncap])
    nr = w.numbers_result()
    arrs = [np.ascontiguousarray(a) for a in (w.idx, w.typ, w.depth, w.match, w.end, w.flags)]
    twins.e.sem_select_elements(blob.ctypes.data, w.data, len(w.data), arrs[0].ctypes.data, w.n, *[a.ctypes.data for a in arrs[1:]],
                                recs.ctypes.data if ncap else None, ncap, ctypes.byref(nr) if numbers_result else None,
                                rows.ctypes.data if rows.size else None, ctypes.byref(rows_select), fields.ctypes.data, capacity,
                                ctypes.byref(res))
    return tsm.Selected(res, fields, len(pointers), capacity)


def record(token, typ="{", bits=0, flags=0, code=0):
    return tac.record(token, typ, bits, flags, code)


# ---- the definition ---------------------------------------------------------------------------------------------------------

def definition(texts, list_pointer, pointers, codes=None):
    """texts: the documents; codes: their verdict codes (None: all 0).  -> (items per document or None where the value at
    `list_pointer` is no list, [[(code, value) per pointer] per row])"""
    per_doc, rows = [], []
    for k, text in enumerate(texts):
        code, v = (codes[k], None) if codes and codes[k] else ref.lookup(ref.decode(text), list_pointer)
        if code != 0 or not isinstance(v, list):
            per_doc.append(None)
            continue
        per_doc.append(v)
        rows += [[ref.lookup(item, pointer) for pointer in pointers] for item in v]
    return per_doc, rows


def check_against_definition(w, got, pointers, rows, bits=True):
    """Every record of `got` (a Selected with room for every row) against the definition's rows -> {(p, r): (code, value)}"""
    R = len(rows)
    data = np.frombuffer(w.data, dtype=np.uint8)
    out, found, no_bits = {}, 0, 0
    for p, pointer in enumerate(pointers):
        col = got.column(p)
        for r in range(R):
            rec, want = col[r], rows[r][p]
            where = (pointer, r, rec, want)
            assert rec["code"] == want[0], where
            if want[0]:
                assert (int(rec["bits"]), int(rec["token"]), int(rec["type"]), int(rec["flags"])) == (0, NO_TOKEN, 0, 0), where
                value = None
            else:
                assert rec["token"] < w.n and chr(int(rec["type"])) in '{["ldtfn', where
                if bits:
                    assert not rec["flags"] & _lib.FIELD_NO_BITS, where
                value = field_value(rec, data, w.idx, w.end)
                assert tsm.same_value(value, want[1]), where + (value,)
                found += 1
                no_bits += bool(rec["flags"] & _lib.FIELD_NO_BITS)
            out[(p, r)] = (want[0], value)
    assert got.summary() == (0, 0, R, len(pointers), found, no_bits, 0), got.summary()
    assert got.untouched(R)
    return out


def check_window(oracle, nm, twins, texts, list_pointer, pointers, verdicts=False, sep=b"\n"):
    """One window the whole way: select twin, array-column twin, element twin, against the definition
    -> (WindowArrays, rows, {(p, r): (code, value)})"""
    w = tdm.WindowArrays(oracle, nm, tdk.join(texts, sep), is_final=True)
    assert w.D == len(texts)
    rows_v = tdm.twin_documents(twins.v, w, 100)[0] if verdicts else None
    lists, rows, esel = element_rows(twins, w, list_pointer, verdicts=rows_v)
    per_doc, want = definition(texts, list_pointer, pointers, [c for c, _ in rows_v] if rows_v else None)
    assert int(lists.res.n_elements) == len(want) == rows.size
    got = twin_elements(twins, w, pointers, rows, esel)
    return w, rows, check_against_definition(w, got, pointers, want)


# ---- a seeded corpus of lists of small objects --------------------------------------------------------------------------------

KEYS = ["sku", "qty", "dims", "a", "é", 'k"q', "", "w"]


def _value(rng, depth=0):
    kind = rng.randrange(9 if depth < 2 else 6)
    if kind == 0:
        return rng.randrange(-1000, 1000)
    if kind == 1:
        return rng.choice([0.5, -2.5e3, 1e-7, 3.0])
    if kind == 2:
        return rng.choice(["", "plain", "e\nsc", "é\U0001F600", 'q"\\/'])
    if kind in (3, 4, 5):
        return rng.choice([None, True, False])
    if kind == 6:
        return {k: _value(rng, depth + 1) for k in rng.sample(["w", "h", "sku", "dims"], rng.randrange(4))}
    if kind == 7:
        return [_item(rng, depth + 1) for _ in range(rng.randrange(3))]
    return {}


def _item(rng, depth=0):
    if rng.randrange(6) == 0:
        return _value(rng, 2)   # an element that is no object
    return {k: _value(rng, depth) for k in rng.sample(KEYS, rng.randrange(len(KEYS)))}


def seeded_lists(seed, n_docs):
    """n_docs lines {"id": k, "items": [...]} -- or something else at items now and then --, a duplicate key spliced into
    some elements; escaped and plain spellings alternate"""
    rng = random.Random(seed)
    out = []
    for k in range(n_docs):
        items = [_item(rng) for _ in range(rng.randrange(7))] if k % 11 else rng.choice([7, {"sku": 1}, None])
        text = json.dumps({"id": k, "items": items}, ensure_ascii=bool(k % 2), separators=(",", ":") if k % 3 else (", ", ": "))
        if k % 5 == 0:
            text = text.replace('{"sku":', '{"sku":"first","sku":', 1)
        out.append(text.encode("utf-8"))
    return out


CORPUS_PATHS = ["/sku", "/qty", "/dims", "/dims/w", "", "/é", '/k"q', "/", "/a", "/dims/dims/w", "/w", "/dims/sku", "/nope"]


# ---- tests ------------------------------------------------------------------------------------------------------------------

def test_corpus_equals_definition(oracle, nm, twins):
    """Seeded lists of small objects, four separators: every (path, element) is the definition's, codes 0, 17 and 20 alike."""
    hist, n_rows = {}, 0
    for j, sep in enumerate((b"\n", b" ", b"\r\n", b"")):
        texts = seeded_lists(4100 + j, 150)
        _, rows, got = check_window(oracle, nm, twins, texts, "/items", CORPUS_PATHS, sep=sep)
        n_rows += rows.size
        for c, _ in got.values():
            hist[c] = hist.get(c, 0) + 1
    assert n_rows > 1200 and all(hist.get(c, 0) > 300 for c in (0, 17, 20)), (n_rows, hist)


def test_pins(oracle, nm, twins):
    """The cases read from the definition, one window with the lists at /items and one with the documents themselves."""
    w, rows, got = check_window(oracle, nm, twins, PINS, "/items", PIN_PATHS)
    col = lambda pointer: [got[(PIN_PATHS.index(pointer), r)] for r in range(rows.size)]
    sku = col("/sku")
    assert sku[:7] == [(0, "a"), (20, None), (17, None), (17, None), (17, None), (20, None), (17, None)]
    assert sku[7] == (0, 2)                                            # {"x":{"sku":1},"sku":2}: not the deeper one
    assert sku[8:10] == [(20, None), (0, 1)]                           # {"a":[{"sku":9}]} has no sku
    assert sku[10:13] == [(0, 1), (0, 3), (0, 4)]                      # the first duplicate; neighbours keep their own
    assert sku[13] == (0, "e\nvé") and col("/qty")[13] == (0, 1.5)   # "sku"
    assert col("/dims/w")[14:19] == [(0, 1), (20, None), (17, None), (20, None), (0, {"w": 3})]
    assert col("/dims/w/w")[14:19] == [(17, None), (20, None), (17, None), (20, None), (0, 3)]
    assert col("/dims")[16] == (0, 5) and col("/qty")[12] == (0, [])
    assert rows.size == 22 and sku[19:21] == [(0, -12), (0, (1 << 63) - 1)] and col("/qty")[19] == (0, 100.0)
    assert col("")[:7] == [(0, {"sku": "a", "qty": 2}), (0, {"qty": 3}), (0, 7), (0, "s"), (0, []), (0, {}), (0, None)]
    assert col("/")[21] == (0, 0) and sku[21] == (0, {})             # the other list of that document contributes no row
    w, rows, got = check_window(oracle, nm, twins, ROOT_PINS, "", ["/sku", ""])
    assert [got[(0, r)] for r in range(rows.size)] == [(0, 2), (20, None), (0, 1), (17, None), (0, [2])]


def test_sixteen_paths(oracle, nm, twins):
    w, rows, got = check_window(oracle, nm, twins, PINS + seeded_lists(7, 40), "/items", SIXTEEN)
    assert rows.size > 100 and sum(c == 0 for c, _ in got.values()) > 200


def test_invalid_documents_contribute_no_rows(oracle, nm, twins):
    """Documents with a verdict code between valid ones: their lists are no rows of the array column, so none of ours; the
    neighbours' rows are exact."""
    texts = [b'{"items":[{"sku":1},{"sku":2}]}', b'{"items":[{"sku":3},tru]}', b'{"items":[{"sku":4}]}', b'{"items":[{"sku":5}],}',
             b'{"items":[{"sku":6,"qty":[1]}]}']
    w, rows, got = check_window(oracle, nm, twins, texts, "/items", ["/sku", "/qty"], verdicts=True)
    assert [got[(0, r)] for r in range(rows.size)] == [(0, 1), (0, 2), (0, 4), (0, 6)] and got[(1, 3)] == (0, [1])


def test_numbers_without_records(oracle, nm, twins):
    """d_numbers NULL, d_numbers_result NULL, or fewer records than a field's: MSJ_FIELD_NO_BITS, bits 0 and the right tag, the
    value from the text; n_found / n_no_bits count them.  With the records: the bits."""
    texts = [b'{"items":[{"i":-12,"f":1.5e2,"s":"x"},{"i":4.25,"f":3}]}', b'{"items":[{"i":9223372036854775807,"f":-0,"z":[1]}]}']
    pointers = ["/i", "/f", "/s", "/z"]
    w, rows, _ = check_window(oracle, nm, twins, texts, "/items", pointers)
    _, want = definition(texts, "/items", pointers)
    full = twin_elements(twins, w, pointers, rows)
    assert [chr(int(t)) for t in full.column(0)[:3]["type"]] == ["l", "d", "l"] and int(full.column(0)[2]["bits"]) == (1 << 63) - 1
    assert (full.res.n_found, full.res.n_no_bits) == (8, 0)
    for kw in (dict(numbers=False), dict(numbers_result=False), dict(numbers_capacity=0)):
        got = twin_elements(twins, w, pointers, rows, **kw)
        check_against_definition(w, got, pointers, want, bits=False)
        assert (got.res.n_found, got.res.n_no_bits) == (8, 6)
        for a, b in zip(got.fields[:12], full.fields[:12]):
            assert (a["type"], a["token"], a["code"]) == (b["type"], b["token"], b["code"])
            assert (int(a["bits"]), int(a["flags"])) == (0, _lib.FIELD_NO_BITS) if chr(int(b["type"])) in "ld" and not b["code"] else a == b
    part = twin_elements(twins, w, pointers, rows, numbers_capacity=4)   # the first document's records only
    check_against_definition(w, part, pointers, want, bits=False)
    assert part.res.n_no_bits == 2 and np.array_equal(part.column(0)[:2], full.column(0)[:2])


def test_head_codes(oracle, nm, twins):
    """d_rows_select with a code (a really clipped element list among them): a zero result with that code.  R > capacity:
    MSJ_CAPACITY, n_documents = R.  R == 0 and n == 0: a result without rows.  Nothing else is written in any."""
    texts = [b'{"items":[{"sku":1},{"sku":2},{"sku":3}]}', b'{"items":[{"sku":4}]}']
    w = tdm.WindowArrays(oracle, nm, tdk.join(texts, b"\n"), is_final=True)
    lists, rows, esel = element_rows(twins, w, "/items")
    clipped, few, csel = element_rows(twins, w, "/items", elements_capacity=3)
    assert csel.code == MSJ_CAPACITY and csel.n_documents == 4 and few.size == 3
    for sel, r in ((csel, few), (rows_result(4, 9), rows), (rows_result(4, -1), rows)):
        got = twin_elements(twins, w, ["/sku", ""], r, sel, capacity=6)
        assert got.summary() == (sel.code, 0, 0, 0, 0, 0, 0) and got.untouched(0)
    for cap in (3, 0):
        got = twin_elements(twins, w, ["/sku", ""], rows, esel, capacity=cap)
        assert got.summary() == (MSJ_CAPACITY, 0, 4, 2, 0, 0, 0) and got.untouched(0)
    none = twin_elements(twins, w, ["/sku", ""], rows[:0], capacity=3)
    assert none.summary() == (0, 0, 0, 2, 0, 0, 0) and none.untouched(0)
    w0 = tdm.WindowArrays(oracle, nm, b"  \n ", is_final=True)
    assert w0.n == 0
    empty = twin_elements(twins, w0, ["/sku", ""], rows[:0], capacity=2)
    assert empty.summary() == (0, 0, 0, 2, 0, 0, 0) and empty.untouched(0)
    # records of another window over a window without a token: no row names a token, "" included
    lost = twin_elements(twins, w0, ["/sku", ""], rows, capacity=5)
    assert lost.summary() == (0, 0, 4, 2, 0, 0, 0) and lost.fields[:4]["code"].tolist() == [17] * 4 and lost.column(1)[:4]["code"].tolist() == [17] * 4
    assert lost.untouched(4)
    assert twins.e.sem_state_rows(0, 5) == 1 and twins.e.sem_state_rows(7, 5) == 5 and twins.e.sem_state_rows(3, 5) == 3


# ---- hostile records ----------------------------------------------------------------------------------------------------------

HOSTILE = [b'{"items":[{"sku":1},{"sku":2},{"sku":3},[4],{"sku":5}]}', b'[{"a":1,"in":{"a":2,"b":3},"b":4}]']


def hostile_window(oracle, nm):
    return tdm.WindowArrays(oracle, nm, tdk.join(HOSTILE, b"\n"), is_final=True)


def codes_and_values(w, got, p, R):
    data = np.frombuffer(w.data, dtype=np.uint8)
    return [(int(r["code"]), field_value(r, data, w.idx, w.end)) for r in got.column(p)[:R]]


def test_descending_pair(oracle, nm, twins):
    """A descending pair anywhere, or two equal tokens: MSJ_ERR_BAD_ARGUMENT, n_documents = R, nothing written."""
    w = hostile_window(oracle, nm)
    _, rows, _ = element_rows(twins, w, "/items")
    assert rows.size == 5 and np.all(np.diff(rows["token"].astype(np.int64)) > 0)
    for a, b in ((0, 1), (3, 4), (1, 3)):
        bad = rows.copy()
        bad[[a, b]] = bad[[b, a]]
        got = twin_elements(twins, w, ["/sku", ""], bad)
        assert got.summary() == (BAD_ARGUMENT, 0, 5, 2, 0, 0, 0) and got.untouched(0), (a, b)
    twice = rows.copy()
    twice[2] = twice[1]
    assert twin_elements(twins, w, ["/sku"], twice).summary() == (BAD_ARGUMENT, 0, 5, 1, 0, 0, 0)
    # compared as uint32: a code's 0xFFFFFFFF is the largest token, and only the last row can have it
    tail = np.concatenate([rows[:2], record(NO_TOKEN, typ="", code=20)])
    assert codes_and_values(w, twin_elements(twins, w, ["/sku"], tail), 0, 3) == [(0, 1), (0, 2), (20, None)]
    head = np.concatenate([record(NO_TOKEN, typ="", code=20), rows[:2]])
    assert twin_elements(twins, w, ["/sku"], head).res.code == BAD_ARGUMENT


def test_records_that_lie(oracle, nm, twins):
    """token >= n; a '{' record on a token that is none; a record of another type on a real object; a partner out of range:
    no lookup, code 17, nothing read out of bounds.  "" re-derives the value from the arrays whatever the record says."""
    w = hostile_window(oracle, nm)
    _, rows, _ = element_rows(twins, w, "/items")
    t = rows["token"].tolist()
    assert [chr(c) for c in w.typ[t]] == list("{{{[{")
    lying = np.concatenate([record(t[0]), record(t[0] + 1), record(t[1], typ="["), record(t[3]), record(t[4], typ='"'),
                            record(w.n), record(w.n + 7), record(NO_TOKEN)])
    got = twin_elements(twins, w, ["/sku", ""], lying)
    assert codes_and_values(w, got, 0, 8) == [(0, 1)] + [(17, None)] * 7
    assert codes_and_values(w, got, 1, 8) == [(0, {"sku": 1}), (0, "sku"), (0, {"sku": 2}), (0, [4]), (0, {"sku": 5})] + [(17, None)] * 3
    assert got.summary() == (0, 0, 8, 2, 6, 0, 0) and got.untouched(8)
    for m in (w.n, w.n + 5, tdk.NO_PARTNER, t[1], t[1] - 1, 0):
        w.match = w.match.copy()
        w.match[t[1]] = m
        got = twin_elements(twins, w, ["/sku"], rows)
        assert codes_and_values(w, got, 0, 5) == [(0, 1), (17, None), (0, 3), (17, None), (0, 5)], m
    typ, mat = np.ascontiguousarray(w.typ), np.ascontiguousarray(w.match)
    state = lambda code, rt, v, levels, n=w.n: twins.e.sem_row_state(code, ord(rt), v, levels, n, typ.ctypes.data, mat.ctypes.data)
    assert state(0, "{", t[0], 1) == t[0] and state(0, "{", t[0], 0) == t[0] and state(0, "[", t[0], 0) == t[0]
    assert state(0, "[", t[0], 1) == 0x80000011 and state(0, "{", t[3], 1) == 0x80000011 and state(0, "{", w.n, 0) == 0x80000011
    assert state(20, "{", t[0], 1) == 0x80000014 and state(9, "{", t[0], 0) == 0x80000009 and state(0, "{", t[0], 1, n=t[0]) == 0x80000011


def test_nested_rows(oracle, nm, twins):
    """Ascending tokens with one row inside another: a key belongs to the LAST row whose token lies below it, and to that
    row alone -- the outer row loses the keys behind the inner row's token, the inner row keeps its own."""
    w = hostile_window(oracle, nm)
    outer = int(w.first[1]) + 1
    assert (chr(w.typ[outer]), chr(w.typ[outer + 1]), chr(w.typ[outer + 7])) == ("{", '"', "{")
    inner = outer + 7
    pointers = ["/a", "/b", "/in", "/in/a", ""]
    nested = twin_elements(twins, w, pointers, np.concatenate([record(outer), record(inner)]))
    cv = lambda got, p: codes_and_values(w, got, p, int(got.res.n_documents))
    assert cv(nested, 0) == [(0, 1), (0, 2)]
    assert cv(nested, 1) == [(20, None), (0, 3)]          # "b":4 lies behind the inner row's token: no longer the outer row's
    assert cv(nested, 2) == [(0, {"a": 2, "b": 3}), (20, None)] and cv(nested, 3) == [(20, None), (20, None)]
    alone = twin_elements(twins, w, pointers, record(outer))
    assert cv(alone, 1) == [(0, 4)] and cv(alone, 3) == [(0, 2)]
    start = np.array([3, 9, 10, 50], dtype=np.uint32)
    below = lambda x, count=4: twins.e.sem_rows_below(start.ctypes.data, count, x)
    assert [below(x) for x in (0, 3, 4, 9, 10, 11, 50, 51, NO_TOKEN)] == [0, 0, 1, 1, 2, 3, 3, 4, 4] and below(99, 0) == 0 and below(99, 2) == 2


def every_token_a_row(n_elements=700):
    """(text, pointers): one array of numbers and {"k":j} objects, more than a block of tokens long"""
    return b"[" + b",".join(b'{"k":%d}' % j if j % 3 == 0 else b"1" for j in range(n_elements)) + b"]\n", ["/k", ""]


def test_every_token_a_row(oracle, nm, twins):
    """Every token of the window is a row, each record claiming an object: the real ones find their key, the rest are 17."""
    text, pointers = every_token_a_row()
    w = tdm.WindowArrays(oracle, nm, text, is_final=True)
    assert w.n > 1025 + 64
    rows = np.concatenate([record(v) for v in range(w.n)])
    got = twin_elements(twins, w, pointers, rows)
    js = iter(range(0, 700, 3))
    want = [(0, next(js)) if w.typ[v] == ord("{") else (17, None) for v in range(w.n)]
    assert sum(c == 0 for c, _ in want) == 234 and codes_and_values(w, got, 0, w.n) == want
    assert got.summary() == (0, 0, w.n, 2, 234 + w.n, 0, 0) and got.untouched(w.n)
