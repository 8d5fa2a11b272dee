"""CPU check of msj_array_elements_device's arithmetic (mojo_simdjson_amd/csrc/array_elements_math.h).

The definition in include/msj_stage1.h is restated in Python from its text alone (`definition` below), on json: per document
the value tests/select_reference.py finds for the list's path; a list gives one parent element per item; for each parent
element the value at the sub-path -- or the element itself -- is looked up by the same reference and is a row; a row that is
a list gives its items.  The host twin (tests/array_elements_math_host.cpp: the verdict on the rows, the live rows, the order
test, the row and element tests of the headers with select_math.h's record, serially) runs over rows that come from the
array-column twin (a list of lists) and from the select-elements twin (a list inside a list of structs); its offsets,
validity bytes and every element record decoded back to a Python value must equal the definition's, fill and canary behind
every array included.  Hostile records -- which json cannot describe -- are pinned by value.  The kernels that run the same
headers on the device are covered by tests/test_array_elements.py (-m gpu).
"""
import ctypes
import json
import os
import random
import subprocess

import numpy as np
import pytest

from mojo_simdjson_amd import _lib
from mojo_simdjson_amd.document_stream import field_value
from tests import helpers
from tests import select_reference as ref
from tests import test_array_column_math as tac
from tests import test_number_math as tnm
from tests import test_select_elements_math as tse
from tests import test_tape_documents_math as tdk
from tests import test_validate_documents_math as tdm
from tests import test_validate_math as tvm

MSJ_CAPACITY, BAD_ARGUMENT = 1, -1
NO_TOKEN = 0xFFFFFFFF

# the elements the definition is pinned on, each the list at /c of one document
PIN_ELEMENTS = [b"[[1,2],[],[3]]", b"[[[1]],[2,[3,4]]]", b'[1,"s",{"a":[9]},[5]]', b'[[{"a":[1]}],[[]]]']
MUTATION_PIN = b"[[1,[2,3]]]"   # without the depth clause of the element test the 2 and the 3 would be elements of the row too
PIN_TEXTS = [b'{"c":' + e + b"}" for e in PIN_ELEMENTS] + [b'{"c":[[],[[],{}],[[1,[2,3]],{"a":[4,5]}]]}', b'{"c":' + MUTATION_PIN + b"}"]
STRUCT_PINS = [b'{"items":[7,{"sku":1},{"tags":["a","b"],"x":{"tags":[0]}},{"sku":2},"s",{"tags":[]},{"tags":[[1],{"tags":[9]}]},{"tags":7},{}]}',
               b'{"items":[{"tags":["c"]},{"x":1}]}', b'{"items":[]}', b'{"items":[{"sku":3},5]}']

_twins = {}


def load_twin(mutation=False):
    """The host twin of the call (g++ build of tests/array_elements_math_host.cpp); mutation: the element test without its
    depth clause."""
    if mutation in _twins:
        return _twins[mutation]
    os.makedirs(tvm.BUILD, exist_ok=True)
    so = os.path.join(tvm.BUILD, "libarray_elements_math_host%s.so" % ("_mutant" if mutation else ""))
    src = os.path.join(helpers.ROOT, "tests", "array_elements_math_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared"] + (["-DMSJ_TWIN_NO_DEPTH_CLAUSE"] if mutation else []) + ["-o", so, src])
    lib = ctypes.CDLL(so)
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    for name, args, res in (("aem_array_elements", [vp, u64] + [vp] * 6 + [u64, vp, vp, vp, vp, vp, u64, vp, u64, vp, vp], None),
                            ("aem_dense_rows", [u64, u64], u64), ("aem_rank_word", [u64, ctypes.c_int], u32),
                            ("aem_offset_of_row", [u32, u64, vp, vp, u64, u64], u64)):
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, res
    _twins[mutation] = lib
    return lib


@pytest.fixture(scope="module")
def oracle():
    return helpers.load_oracle()


@pytest.fixture(scope="module")
def nm():
    return tnm.load_twin()


@pytest.fixture(scope="module")
def twins():
    t = tse.Twins()
    t.l = load_twin()
    return t


# ---- the twin ---------------------------------------------------------------------------------------------------------------

def twin_lists(ltwin, w, rows, rows_select=None, capacity=None, elements_capacity=None, layout_only=False, numbers=True, numbers_result=True,
               numbers_capacity=None):
    """aem_array_elements over the window's arrays and the records `rows`.  rows_select None: a result for len(rows) rows.
    elements_capacity None: what a layout-only first call reports.  numbers False: d_numbers NULL with capacity 0;
    numbers_result False: d_numbers_result NULL.  -> tac.Lists"""
    rows = np.ascontiguousarray(rows)
    rows_select = tse.rows_result(rows.size) if rows_select is None else rows_select
    capacity = max(rows.size, 1) if capacity is None else capacity
    kw = dict(rows_select=rows_select, capacity=capacity, numbers=numbers, numbers_result=numbers_result, numbers_capacity=numbers_capacity)
    if elements_capacity is None and not layout_only:
        elements_capacity = int(twin_lists(ltwin, w, rows, layout_only=True, **kw).res.n_elements)
    room = 0 if layout_only else elements_capacity
    offsets, valid, elements = tac.filled(capacity, room, layout_only)
    res, esel = _lib.MsjArrayColumnResult(), _lib.MsjSelectDocumentsResult()
    ncap = (int(w.records.size) if numbers_capacity is None else numbers_capacity) if numbers else 0
    recs = np.ascontiguousarray(w.records[:ncap])
    nr = w.numbers_result()
    arrs = [np.ascontiguousarray(a) for a in (w.idx, w.typ, w.depth, w.match, w.end, w.flags)]
    ltwin.aem_array_elements(arrs[0].ctypes.data, w.n, *[a.ctypes.data for a in arrs[1:]], recs.ctypes.data if ncap else None, ncap,
                             ctypes.byref(nr) if numbers_result else None, rows.ctypes.data if rows.size else None, ctypes.byref(rows_select),
                             offsets.ctypes.data, valid.ctypes.data, capacity, elements.ctypes.data if elements is not None else None, room,
                             ctypes.byref(res), ctypes.byref(esel))
    return tac.Lists(res, esel, offsets, valid, elements, capacity, room)


def record(token, typ="[", bits=0, flags=0, code=0):
    return tac.record(token, typ, bits, flags, code)


def coded(code):
    """A record as the select calls write it for a lookup that failed"""
    return record(NO_TOKEN, typ="", code=code)


def parent_rows(twins, w, list_pointer, sub=None, verdicts=None):
    """The rows of one window: the element records of the list at `list_pointer` (sub None), or the records of the pointer
    `sub` looked up in those elements -> (records, their msj_select_documents_result)"""
    _, rows, esel = tse.element_rows(twins, w, list_pointer, verdicts=verdicts)
    if sub is None:
        return rows, esel
    got = tse.twin_elements(twins, w, [sub], rows, esel)
    return got.column(0)[:rows.size].copy(), got.res


def next_level(lists):
    """A twin's complete output as the next call's rows"""
    return lists.elements[:int(lists.res.n_elements)].copy(), lists.esel


# ---- the definition ---------------------------------------------------------------------------------------------------------

def definition(texts, list_pointer, sub=None, codes=None):
    """texts: the documents; codes: their verdict codes (None: all 0).  -> [(code, value) per row]: a row per item of every
    document's list at `list_pointer`, the item itself or what `sub` finds in it"""
    rows = []
    for k, text in enumerate(texts):
        code, v = (codes[k], None) if codes and codes[k] else ref.lookup(ref.decode(text), list_pointer)
        if code == 0 and isinstance(v, list):
            rows += [(0, item) if sub is None else ref.lookup(item, sub) for item in v]
    return rows


def items_of(values):
    """The next level's rows: the items of the rows that are lists"""
    return [(0, item) for code, v in values if code == 0 and isinstance(v, list) for item in v]


def check_window(oracle, nm, twins, texts, list_pointer, sub=None, verdicts=False, sep=b"\n"):
    """One window the whole way: rows from the sibling twins, this twin in the layout-only form and complete, against the
    definition -> (WindowArrays, rows, rows_select, the complete tac.Lists, [(code, value) per row])"""
    w = tdm.WindowArrays(oracle, nm, tdk.join(texts, sep), is_final=True)
    assert w.D == len(texts)
    rows_v = tdm.twin_documents(twins.v, w, 100)[0] if verdicts else None
    rows, rsel = parent_rows(twins, w, list_pointer, sub, verdicts=rows_v)
    values = definition(texts, list_pointer, sub, [c for c, _ in rows_v] if rows_v else None)
    assert rows.size == len(values)
    full = twin_lists(twins.l, w, rows, rsel)
    tac.check_against_definition(w, full, values)
    layout = twin_lists(twins.l, w, rows, rsel, layout_only=True)
    assert layout.summary() == full.summary() and layout.elements is None
    assert np.array_equal(layout.offsets, full.offsets) and np.array_equal(layout.valid, full.valid)
    return w, rows, rsel, full, values


# ---- a seeded corpus of lists of lists and of lists of structs with lists ----------------------------------------------------

def _scalar(rng):
    return rng.choice([rng.randrange(-1000, 1000), 0.5, -2.5e3, "", "plain", "e\nsc", "é\U0001F600", None, True, False])


def _list(rng, depth=0):
    out = []
    for _ in range(rng.randrange(5)):
        kind = rng.randrange(8 if depth < 3 else 4)
        if kind < 4:
            out.append(_scalar(rng))
        elif kind < 6:
            out.append(_list(rng, depth + 1))
        elif kind == 6:
            out.append({"a": _list(rng, depth + 1), "b": _scalar(rng)})
        else:
            out.append(rng.choice([[], {}]))
    return out


def _struct(rng):
    kind = rng.randrange(8)
    if kind == 0:
        return _scalar(rng)            # an element that is no object: 17
    if kind == 1:
        return {"sku": _scalar(rng)}   # no tags: 20
    tags = _list(rng, 1) if kind < 6 else rng.choice([7, "t", {"tags": [1]}, None])
    return {"sku": _scalar(rng), "x": {"tags": [0]}, "tags": tags, "after": [_scalar(rng)]}


def seeded_documents(seed, n_docs):
    """n_docs lines {"id": k, "c": [lists ...], "items": [structs with "tags" ...]} -- or something else at c / items now and
    then; escaped and plain spellings, compact and spaced separators alternate"""
    rng = random.Random(seed)
    out = []
    for k in range(n_docs):
        c = _list(rng) if k % 9 else rng.choice([7, {"c": [1]}, None, []])
        items = [_struct(rng) for _ in range(rng.randrange(6))] if k % 11 else rng.choice([7, {"tags": [1]}])
        doc = {"id": k, "c": c, "items": items}
        out.append(json.dumps(doc, ensure_ascii=bool(k % 2), separators=(",", ":") if k % 3 else (", ", ": ")).encode("utf-8"))
    return out


# ---- tests ------------------------------------------------------------------------------------------------------------------

def test_corpus_equals_definition(oracle, nm, twins):
    """Seeded documents under the four separators: the list of lists at /c and the lists at /tags inside the structs of
    /items, rows that are arrays, other values and codes 17 and 20 alike."""
    arrays = elements = coded_rows = 0
    for j, sep in enumerate((b"\n", b" ", b"\r\n", b"")):
        texts = seeded_documents(5200 + j, 120)
        for list_pointer, sub in (("/c", None), ("/items", "/tags"), ("/items", ""), ("/items", "/x/tags")):
            _, rows, _, full, values = check_window(oracle, nm, twins, texts, list_pointer, sub, sep=sep)
            arrays, elements = arrays + int(full.res.n_arrays), elements + int(full.res.n_elements)
            coded_rows += sum(c != 0 for c, _ in values)
    assert arrays > 1000 and elements > 2000 and coded_rows > 200, (arrays, elements, coded_rows)


def test_pins(oracle, nm, twins):
    """The cases read from the definition: the pinned elements; rows that are []; a nested [] / {} as an element; the contents
    of nested containers not counted; rows from several documents."""
    w, rows, _, full, values = check_window(oracle, nm, twins, PIN_TEXTS, "/c")
    offsets, valid, items = tac.definition(values)[:3]
    per_row = [items[offsets[r]:offsets[r + 1]] if valid[r] else None for r in range(len(values))]
    assert per_row[:3] == [[1, 2], [], [3]]
    assert per_row[3:5] == [[[1]], [2, [3, 4]]]
    assert per_row[5:9] == [None, None, None, [5]]
    assert per_row[9:11] == [[{"a": [1]}], [[]]]
    assert per_row[11:14] == [[], [[], {}], [[1, [2, 3]], {"a": [4, 5]}]]
    assert per_row[14] == [1, [2, 3]] and len(per_row) == 15
    assert full.res.n_other == 3 and full.res.n_arrays == 12
    # one mutation, shown to fail: without `d_depth[i] == d_depth[v] + 1` the 2 and the 3 of [[1,[2,3]]] are elements too
    alone = tdm.WindowArrays(oracle, nm, b'{"c":' + MUTATION_PIN + b"}\n", is_final=True)
    r1, s1 = parent_rows(twins, alone, "/c")
    assert int(twin_lists(twins.l, alone, r1, s1).res.n_elements) == 2
    assert int(twin_lists(load_twin(mutation=True), alone, r1, s1).res.n_elements) == 4


def test_list_inside_a_list_of_structs(oracle, nm, twins):
    """items[*].tags: rows with codes 20 and 17 at the front, at the end and between live rows have no element and the next
    row's offset; a deeper "tags" and one in a nested array are not the row's."""
    w, rows, rsel, full, values = check_window(oracle, nm, twins, STRUCT_PINS, "/items", "/tags")
    assert [c for c, _ in values] == [17, 20, 0, 20, 17, 0, 0, 0, 20, 0, 20, 20, 17]
    assert rows["token"][[0, 1, 3, 4, 8, 10, 11, 12]].tolist() == [NO_TOKEN] * 8
    assert full.offsets[:14].tolist() == [0, 0, 0, 2, 2, 2, 2, 4, 4, 4, 5, 5, 5, 5]
    assert full.valid[:13].tolist() == [0, 0, 1, 0, 0, 1, 1, 0, 0, 1, 0, 0, 0] and (full.res.n_arrays, full.res.n_other) == (4, 1)
    data = np.frombuffer(w.data, dtype=np.uint8)
    assert [field_value(r, data, w.idx, w.end) for r in full.elements[:5]] == ["a", "b", [1], {"tags": [9]}, "c"]
    # every row has a code: no live row at all
    none = twin_lists(twins.l, w, np.concatenate([coded(20), coded(17), coded(20)]))
    assert none.summary()[:7] == (0, 0, 3, 0, 0, 0, 0) and none.offsets[:4].tolist() == [0] * 4 and none.valid[:3].tolist() == [0] * 3
    assert none.untouched(3, 0)


def test_invalid_documents_contribute_no_rows(oracle, nm, twins):
    """Documents with a verdict code between valid ones: their lists are no rows of the parent column, so none of ours."""
    texts = [b'{"c":[[1],[2,3]]}', b'{"c":[[4],tru]}', b'{"c":[[5]]}', b'{"c":[[6]],}', b'{"c":[[7,[8]]]}']
    _, rows, _, full, _ = check_window(oracle, nm, twins, texts, "/c", verdicts=True)
    assert rows.size == 4 and full.offsets[:5].tolist() == [0, 1, 3, 4, 6]


def test_three_levels_deep(oracle, nm, twins):
    """The call applied to its own output: [[[[1,2],[3]],[[4]]],[],[[[5,[6]]],7]] three times over, each level against
    json."""
    texts = [b"[[[[1,2],[3]],[[4]]],[],[[[5,[6]]],7]]", b"[[[[8]]]]", b"[1]"]
    w = tdm.WindowArrays(oracle, nm, tdk.join(texts, b"\n"), is_final=True)
    rows, rsel = parent_rows(twins, w, "")
    values = definition(texts, "")
    seen = []
    for level in range(3):
        full = twin_lists(twins.l, w, rows, rsel)
        tac.check_against_definition(w, full, values)
        seen.append((int(full.res.n_rows), int(full.res.n_arrays), int(full.res.n_elements)))
        (rows, rsel), values = next_level(full), items_of(values)
    assert seen == [(5, 4, 5), (5, 4, 5), (5, 5, 7)]   # (rows, arrays, elements) as counted by hand from the texts
    assert [v for _, v in values] == [1, 2, 3, 4, 5, [6], 8]


def test_numbers_without_records(oracle, nm, twins):
    """d_numbers NULL, d_numbers_result NULL, or fewer records than an element's: MSJ_FIELD_NO_BITS, bits 0 and the right
    tag, counted only where written; the value comes from the text.  With the records: the bits."""
    texts = [b'{"c":[[-12,1.5e2,"x",0.0],[3,[4.25],9223372036854775807]]}', b'{"c":[[-0,{"n":1}]]}']
    w, rows, rsel, full, values = check_window(oracle, nm, twins, texts, "/c")
    assert [chr(int(t)) for t in full.elements[:9]["type"]] == list('ld"dl[ll{') and int(full.elements[6]["bits"]) == (1 << 63) - 1
    for kw in (dict(numbers=False), dict(numbers_result=False), dict(numbers_capacity=0)):
        part = twin_lists(twins.l, w, rows, rsel, **kw)
        tac.check_against_definition(w, part, values, bits=False)
        assert part.res.n_no_bits == 6
        for a, b in zip(part.elements[:9], full.elements[:9]):
            assert (a["type"], a["token"], a["code"]) == (b["type"], b["token"], b["code"])
            assert (int(a["bits"]), int(a["flags"])) == (0, _lib.FIELD_NO_BITS) if chr(int(b["type"])) in "ld" else a == b
    few = twin_lists(twins.l, w, rows, rsel, numbers_capacity=3)    # the first row's records only
    tac.check_against_definition(w, few, values, bits=False)
    assert few.res.n_no_bits == 3 and np.array_equal(few.elements[:4], full.elements[:4])
    clipped = twin_lists(twins.l, w, rows, rsel, numbers=False, elements_capacity=2)
    assert clipped.res.n_no_bits == 2 and clipped.res.code == MSJ_CAPACITY    # (only the records written count)


def test_head_codes_and_capacities(oracle, nm, twins):
    """d_rows_select with a code (a really clipped parent list among them): a zero result with that code.  R > capacity:
    MSJ_CAPACITY, n_rows = R.  R == 0 and n == 0: offsets[0] = 0 and a zero result.  elements_capacity short: offsets and
    validity complete, the elements clipped, n_elements exact."""
    texts = [b'{"c":[[1,2],[3],[]]}', b'{"c":[[4,[5]]]}']
    w = tdm.WindowArrays(oracle, nm, tdk.join(texts, b"\n"), is_final=True)
    _, rows, esel = tse.element_rows(twins, w, "/c")
    _, few, csel = tse.element_rows(twins, w, "/c", elements_capacity=3)
    assert csel.code == MSJ_CAPACITY and csel.n_documents == 4 and few.size == 3
    for sel, r in ((csel, few), (tse.rows_result(4, 9), rows), (tse.rows_result(4, -1), rows)):
        got = twin_lists(twins.l, w, r, sel, capacity=6, elements_capacity=8)
        assert got.summary() == (sel.code, 0, 0, 0, 0, 0, 0, sel.code, 0, 0, 1, 0, 0, 0) and got.untouched(-1, 0)
    for cap in (3, 0):
        got = twin_lists(twins.l, w, rows, esel, capacity=cap, elements_capacity=8)
        assert got.summary() == (MSJ_CAPACITY, 0, 4, 0, 0, 0, 0, MSJ_CAPACITY, 0, 0, 1, 0, 0, 0) and got.untouched(-1, 0)
    full = twin_lists(twins.l, w, rows, esel, capacity=6)
    assert full.summary() == (0, 0, 4, 4, 5, 0, 0, 0, 0, 5, 1, 5, 0, 0) and full.offsets[:5].tolist() == [0, 2, 3, 3, 5] and full.untouched(4, 5)
    for room in (4, 0, 2):
        clip = twin_lists(twins.l, w, rows, esel, capacity=6, elements_capacity=room)
        assert clip.summary() == (MSJ_CAPACITY, 0, 4, 4, 5, 0, 0, MSJ_CAPACITY, 0, 5, 1, 5, 0, 0) and clip.untouched(4, room)
        assert np.array_equal(clip.offsets, full.offsets) and np.array_equal(clip.valid, full.valid)
        assert np.array_equal(clip.elements[:room], full.elements[:room])
    for cap in (3, 0):
        none = twin_lists(twins.l, w, rows[:0], capacity=cap, elements_capacity=2)
        assert none.summary() == (0,) * 10 + (1, 0, 0, 0) and none.untouched(0, 0) and (cap == 0 or none.offsets[0] == 0)
    w0 = tdm.WindowArrays(oracle, nm, b"  \n ", is_final=True)
    assert w0.n == 0
    empty = twin_lists(twins.l, w0, rows[:0], capacity=2, elements_capacity=2)
    assert empty.summary() == (0,) * 10 + (1, 0, 0, 0) and empty.offsets[0] == 0 and empty.untouched(0, 0)
    # records of another window over a window without a token: no row is valid
    lost = twin_lists(twins.l, w0, rows, capacity=5, elements_capacity=2)
    assert lost.summary() == (0, 0, 4, 0, 0, 4, 0, 0, 0, 0, 1, 0, 0, 0) and lost.offsets[:5].tolist() == [0] * 5 and lost.valid[:4].tolist() == [0] * 4
    assert twins.l.aem_dense_rows(0, 5) == 0 and twins.l.aem_dense_rows(7, 5) == 5 and twins.l.aem_dense_rows(3, 5) == 3


# ---- hostile records ----------------------------------------------------------------------------------------------------------

#            0 1 2 3 4 5 6 7 8 9 10 12 14 15 17 18    19 20 22 23
HOSTILE = b"[ [ 1 , 2 ] , [ 3 , [ 4,5 ]  ]  ,6 ]  \n  [  [ 7 ]  ]\n"
OUTER, FIRST, SECOND, INNER, OTHER, LAST = 0, 1, 7, 10, 19, 20   # the '[' tokens; n = 24


def hostile_window(oracle, nm):
    w = tdm.WindowArrays(oracle, nm, HOSTILE, is_final=True)
    assert w.n == 24 and [v for v in range(w.n) if w.typ[v] == ord("[")] == [OUTER, FIRST, SECOND, INNER, OTHER, LAST]
    return w


def tokens_per_row(got):
    R = int(got.res.n_rows)
    off = got.offsets[:R + 1].tolist()
    return [got.elements[off[r]:off[r + 1]]["token"].tolist() if got.valid[r] else None for r in range(R)]


def test_order_violations(oracle, nm, twins):
    """A descending or equal pair of live rows anywhere, also with coded rows between them: MSJ_ERR_BAD_ARGUMENT, n_rows = R,
    every count 0, nothing written -- neither d_valid nor d_offsets.  Coded rows anywhere between ascending live rows: fine."""
    w = hostile_window(oracle, nm)
    good = [record(FIRST), record(SECOND), record(OTHER), record(LAST)]
    assert tokens_per_row(twin_lists(twins.l, w, np.concatenate(good))) == [[2, 4], [8, 10], [20], [21]]
    for order in ([1, 0, 2, 3], [0, 1, 3, 2], [0, 2, 1, 3], [3, 0, 1, 2], [0, 1, 2, 2], [0, 0, 1, 2]):
        for gap in ([], [coded(20)], [coded(17), coded(20), coded(20)]):
            rows = []
            for j in order:
                rows += [good[j]] + gap
            rows = np.concatenate(gap + rows)
            got = twin_lists(twins.l, w, rows, elements_capacity=8)
            assert got.summary() == (BAD_ARGUMENT, 0, rows.size, 0, 0, 0, 0, BAD_ARGUMENT, 0, 0, 1, 0, 0, 0), (order, len(gap))
            assert got.untouched(-1, 0), (order, len(gap))
    for gap in ([coded(20)], [coded(17), coded(20), coded(20)]):
        rows = []
        for g in good:
            rows += gap + [g] + gap
        got = twin_lists(twins.l, w, np.concatenate(rows))
        assert [t for t in tokens_per_row(got) if t is not None] == [[2, 4], [8, 10], [20], [21]] and got.res.code == 0
    # compared as uint32, and only among the live rows: a LIVE 0xFFFFFFFF is the largest token and can only be the last live row
    tail = np.concatenate(good + [record(NO_TOKEN), coded(20)])
    assert twin_lists(twins.l, w, tail).summary()[:7] == (0, 0, 6, 4, 6, 1, 0)
    head = np.concatenate([record(NO_TOKEN)] + good)
    assert twin_lists(twins.l, w, head, elements_capacity=8).res.code == BAD_ARGUMENT


def test_records_that_lie(oracle, nm, twins):
    """token >= n; a '[' record on a token that is none; a record of another type on a real array; a partner out of range: no
    array, no element, nothing read out of bounds -- and the row still owns its tokens: it is live."""
    w = hostile_window(oracle, nm)
    lying = np.concatenate([record(OUTER, typ="{"), record(FIRST), record(2), record(SECOND, typ='"'), record(INNER), coded(17), record(OTHER + 2),
                            record(w.n), record(w.n + 7), record(NO_TOKEN)])
    got = twin_lists(twins.l, w, lying)
    assert tokens_per_row(got) == [None, [2], None, None, [11, 13], None, None, None, None, None]   # (token 4 belongs to the row at 2)
    assert got.offsets[:11].tolist() == [0, 0, 1, 1, 1, 3, 3, 3, 3, 3, 3] and (got.res.n_arrays, got.res.n_other) == (2, 7)
    assert got.untouched(10, 3)
    rows = np.concatenate([record(FIRST), record(SECOND), record(OTHER)])
    for m in (w.n, w.n + 5, tdk.NO_PARTNER, SECOND, SECOND - 1, 0):
        w.match = w.match.copy()
        w.match[SECOND] = m
        got = twin_lists(twins.l, w, rows)
        assert tokens_per_row(got) == [[2, 4], None, [20]] and got.res.n_other == 1, m


def test_row_inside_a_row(oracle, nm, twins):
    """Ascending tokens with one row inside another: a token belongs to the LAST live row below it, and to that row alone --
    the outer row keeps the tokens up to and including the inner row's own, the inner row the rest."""
    w = hostile_window(oracle, nm)
    alone = twin_lists(twins.l, w, record(OUTER))
    assert tokens_per_row(alone) == [[FIRST, SECOND, 17]]
    nested = twin_lists(twins.l, w, np.concatenate([record(OUTER), record(SECOND)]))
    assert tokens_per_row(nested) == [[FIRST, SECOND], [8, INNER]] and nested.offsets[:3].tolist() == [0, 2, 4]   # 17 is nobody's
    # a coded row between them changes nothing; a live row that is no array takes the tokens all the same
    assert tokens_per_row(twin_lists(twins.l, w, np.concatenate([record(OUTER), coded(20), record(SECOND)]))) == [[FIRST, SECOND], None, [8, INNER]]
    assert tokens_per_row(twin_lists(twins.l, w, np.concatenate([record(OUTER), record(3)]))) == [[FIRST], None]
    word = twins.l.aem_rank_word
    assert word(0, 1) == 0x80000000 and word(5, 0) == 5 and word(1 << 40, 1) == 0xFFFFFFFF and word((1 << 31) - 1, 0) == 0x7FFFFFFF
    start, doff = np.array([3, 9, 30], dtype=np.uint32), np.array([1, 4, 99], dtype=np.uint64)
    off = lambda word, dense=3, n=24: twins.l.aem_offset_of_row(word, dense, start.ctypes.data, doff.ctypes.data, n, 7)
    assert [off(0), off(0x80000001), off(2), off(3), off(1, dense=1), off(0x7FFFFFFF)] == [1, 4, 7, 7, 7, 7]


def every_token_a_row(n_arrays=600):
    """A window of [k] arrays inside one array, more than two blocks of tokens long"""
    return b"[" + b",".join(b"[%d]" % j if j % 3 else b"[]" for j in range(n_arrays)) + b"]\n"


def test_every_token_a_row(oracle, nm, twins):
    """Every token of the window is a row, each record claiming an array: a row owns the one token behind it, so the real
    arrays keep their first element when it sits there, and the rest are no arrays."""
    w = tdm.WindowArrays(oracle, nm, every_token_a_row(), is_final=True)
    assert w.n > 2048 + 64
    rows = np.concatenate([record(v) for v in range(w.n)])
    got = twin_lists(twins.l, w, rows)
    want = [[v + 1] if w.typ[v] == ord("[") and w.typ[v + 1] != ord("]") else ([] if w.typ[v] == ord("[") else None) for v in range(w.n)]
    assert tokens_per_row(got) == want and got.res.n_arrays == 601 and got.res.n_elements == 1 + 400
    assert got.untouched(w.n, 401)
