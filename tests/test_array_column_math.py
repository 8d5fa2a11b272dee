"""CPU check of msj_array_column_device's arithmetic (mojo_simdjson_amd/csrc/array_column_math.h).

The definition in include/msj_stage1.h is restated in Python from its text alone (`definition` below): per document the
value tests/select_reference.py finds for the path -- a list gives its items, anything else is no array.  The host twin
(tests/array_column_math_host.cpp: the row test, the element test, the code rule of the header and select_math.h's record,
serially) runs over the records of the select twin (tests/test_select_math.py); its offsets, validity bytes and every
element record decoded back to a Python value must equal the definition's, fill and canary behind every array included.
The kernels that run the same header on the device are covered by tests/test_array_column.py (-m gpu).
"""
import ctypes
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
from tests import test_select_math as tsm
from tests import test_tape_documents_math as tdk
from tests import test_validate_documents_math as tdm
from tests import test_validate_math as tvm

MSJ_CAPACITY, BAD_ARGUMENT = 1, -1
FILL = 0x77
CANARY = 64         # bytes behind every array
PINS = [b"[]", b"[[],[]]", b"[{}]", b"[[1,2],[3]]", b'[{"a":[1,2]},3]', b'{"a":[1,"x\\n",null,true,2.5,{"b":[7]}]}', b'{"b":[1]}', b"7",
        b'{"a":{"b":[7]}}', b'"s"', b'{"a":[[[]],[],{"a":[]}]}']

_twin = None


def load_twin():
    """The host twin of the call (g++ build of tests/array_column_math_host.cpp)."""
    global _twin
    if _twin is not None:
        return _twin
    os.makedirs(tvm.BUILD, exist_ok=True)
    so = os.path.join(tvm.BUILD, "libarray_column_math_host.so")
    src = os.path.join(helpers.ROOT, "tests", "array_column_math_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    for name, args, res in (("acm_array_column", [vp, u64] + [vp] * 8 + [u64, vp, vp, vp, vp, vp, u64, vp, u64, vp, vp], None),
                            ("acm_is_candidate", [u32, u32], ctypes.c_int),
                            ("acm_row", [vp, ctypes.c_int, u64, u64, vp, vp, vp, vp, vp, vp], ctypes.c_int)):
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
    return tsm.load_twin()


@pytest.fixture(scope="module")
def atwin():
    return load_twin()


# ---- the twin ---------------------------------------------------------------------------------------------------------------

class Lists:
    """What one call left: the two results and the three arrays, each with its fill and 64 bytes of canary behind its
    capacity.  elements is None in the layout-only form."""

    def __init__(self, res, esel, offsets, valid, elements, capacity, elements_capacity):
        self.res, self.esel, self.offsets, self.valid, self.elements = res, esel, offsets, valid, elements
        self.capacity, self.elements_capacity = capacity, elements_capacity

    def summary(self):
        r, e = self.res, self.esel
        return (r.code, r.flags, r.n_rows, r.n_arrays, r.n_elements, r.n_other, r.n_no_bits,
                e.code, e.flags, e.n_documents, e.n_paths, e.n_found, e.n_no_bits, e.reserved)

    def untouched(self, rows, n_elements):
        """Offsets past `rows` (-1: none written at all), validity bytes at or past it, element records at or past
        `n_elements`, and the canaries, are as they were filled"""
        ok = bool((self.offsets.view(np.uint8)[8 * (rows + 1):] == FILL).all()) and bool((self.valid[max(rows, 0):] == FILL).all())
        return ok and (self.elements is None or bool((self.elements.view(np.uint8)[16 * n_elements:] == FILL).all()))


def filled(capacity, elements_capacity, layout_only=False):
    """-> (offsets uint64[capacity + 1 + 8], valid uint8[capacity + 64], elements FIELD_DTYPE[elements_capacity + 4] or None)"""
    offsets = np.full(8 * (capacity + 1) + CANARY, FILL, dtype=np.uint8).view(np.uint64)
    valid = np.full(capacity + CANARY, FILL, dtype=np.uint8)
    elements = None if layout_only else np.full(16 * elements_capacity + CANARY, FILL, dtype=np.uint8).view(FIELD_DTYPE)
    return offsets, valid, elements


def select_result(D, code=0, n_paths=1):
    return _lib.MsjSelectDocumentsResult(code, 0, D, n_paths, 0, 0, 0)


def twin_lists(atwin, w, records, sel_D=None, sel_code=0, capacity=None, elements_capacity=None, layout_only=False, numbers=True,
               numbers_result=True, numbers_capacity=None):
    """acm_array_column over the window's arrays and `records` (FIELD_DTYPE, one path's column).  elements_capacity None:
    what a layout-only first call reports.  numbers False: d_numbers NULL with capacity 0; numbers_result False:
    d_numbers_result NULL.  -> Lists"""
    capacity = max(w.D, 1) if capacity is None else capacity
    kw = dict(sel_D=sel_D, sel_code=sel_code, capacity=capacity, numbers=numbers, numbers_result=numbers_result, numbers_capacity=numbers_capacity)
    if elements_capacity is None and not layout_only:
        elements_capacity = int(twin_lists(atwin, w, records, layout_only=True, **kw).res.n_elements)
    room = 0 if layout_only else elements_capacity
    records = np.ascontiguousarray(records)
    sel = select_result(w.D if sel_D is None else sel_D, sel_code)
    offsets, valid, elements = filled(capacity, room, layout_only)
    docs = _lib.MsjDocumentsResult(*w.docs)
    res, esel = _lib.MsjArrayColumnResult(), _lib.MsjSelectDocumentsResult()
    ncap = (int(w.records.size) if numbers_capacity is None else numbers_capacity) if numbers else 0
    recs = np.ascontiguousarray(w.records[:ncap])
    nr = w.numbers_result()
    arrs = [np.ascontiguousarray(a) for a in (w.idx, w.typ, w.depth, w.match, w.end, w.flags, w.first)]
    atwin.acm_array_column(arrs[0].ctypes.data, w.n, *[a.ctypes.data for a in arrs[1:]], ctypes.byref(docs), recs.ctypes.data if ncap else None,
                           ncap, ctypes.byref(nr) if numbers_result else None, records.ctypes.data, ctypes.byref(sel), offsets.ctypes.data,
                           valid.ctypes.data, capacity, elements.ctypes.data if elements is not None else None, room, ctypes.byref(res),
                           ctypes.byref(esel))
    return Lists(res, esel, offsets, valid, elements, capacity, room)


def record(token, typ="[", bits=0, flags=0, code=0):
    rec = np.zeros(1, dtype=FIELD_DTYPE)
    rec["bits"], rec["token"], rec["type"], rec["flags"], rec["code"] = bits, token, ord(typ) if typ else 0, flags, code
    return rec


# ---- the definition ---------------------------------------------------------------------------------------------------------

def definition(values):
    """values: (code, Python value) per document, as tests/select_reference.py gives them for the path (a document with a
    verdict code: (its code, None)).  -> (offsets, valid, items, n_other)"""
    offsets, valid, items, n_other = [0], [], [], 0
    for code, v in values:
        is_array = code == 0 and isinstance(v, list)
        valid.append(int(is_array))
        n_other += code == 0 and not is_array
        if is_array:
            items += v
        offsets.append(len(items))
    return offsets, valid, items, n_other


def check_against_definition(w, got, values, bits=True):
    """A twin's (or the device's) complete column -- room for every row and every element -- against the definition"""
    offsets, valid, items, n_other = definition(values)
    D = len(values)
    assert got.offsets[:D + 1].tolist() == offsets and got.valid[:D].tolist() == valid
    data = np.frombuffer(w.data, dtype=np.uint8)
    no_bits = 0
    for j, want in enumerate(items):
        r = got.elements[j]
        assert r["code"] == 0 and chr(int(r["type"])) in '{["ldtfn', (j, r)
        if bits:
            assert not r["flags"] & _lib.FIELD_NO_BITS, (j, r)
        no_bits += bool(r["flags"] & _lib.FIELD_NO_BITS)
        value = field_value(r, data, w.idx, w.end)
        assert tsm.same_value(value, want), (j, r, value, want)
    n = len(items)
    assert got.summary() == (0, 0, D, sum(valid), n, n_other, no_bits, 0, 0, n, 1, n, no_bits, 0), got.summary()
    assert got.untouched(D, n)
    return offsets, valid, items


def column_values(w, stwin, pointers, docs, verdicts=None, **kw):
    """The select twin's records of every pointer, held against the reference -> (Selected, {(p, k): (code, value)})"""
    got = tsm.twin_select(stwin, w, pointers, verdicts=verdicts, **kw)
    values = tsm.check_against_reference(w, got, pointers, docs, codes=[c for c, _ in verdicts] if verdicts else None,
                                         bits=kw.get("numbers", True) and kw.get("numbers_result", True) and "numbers_capacity" not in kw)
    return got, values


def check_window(w, stwin, atwin, pointers, docs, verdicts=None):
    """Every pointer's column of one window: the layout-only form and the complete one against the definition
    -> [(arrays, elements) per pointer]"""
    got, values = column_values(w, stwin, pointers, docs, verdicts)
    out = []
    for p in range(len(pointers)):
        records = got.column(p)[:w.D].copy()
        vals = [values[(p, k)] for k in range(w.D)]
        full = twin_lists(atwin, w, records)
        _, valid, items = check_against_definition(w, full, vals)
        layout = twin_lists(atwin, w, records, layout_only=True)
        assert layout.summary() == full.summary() and layout.elements is None
        assert np.array_equal(layout.offsets, full.offsets) and np.array_equal(layout.valid, full.valid)
        out.append((sum(valid), len(items)))
    return out


# ---- tests ------------------------------------------------------------------------------------------------------------------

def test_corpus_equals_definition(oracle, nm, stwin, atwin):
    """The select corpus with paths drawn from each stream's keys, the root among them: offsets, validity and every element
    are the definition's."""
    arrays = elements = 0
    for j, (data, docs, pointers) in enumerate(tsm.corpus()):
        w = tdm.WindowArrays(oracle, nm, data, is_final=True)
        assert w.D == len(docs)
        for a, e in check_window(w, stwin, atwin, pointers, docs):
            arrays, elements = arrays + a, elements + e
    assert arrays > 500 and elements > 1000, (arrays, elements)   # (what the definition counts in the corpus)


def test_pins(oracle, nm, stwin, atwin):
    """The cases read from the definition, one window: the root array through "", a key, a missing key, a scalar."""
    pointers = ["", "/a", "/a/b", "/zz"]
    w = tdm.WindowArrays(oracle, nm, tdk.join(PINS, b"\n"), is_final=True)
    assert w.D == len(PINS)
    got, values = column_values(w, stwin, pointers, PINS)
    rows = {}
    for p, pointer in enumerate(pointers):
        full = twin_lists(atwin, w, got.column(p)[:w.D].copy())
        offsets, valid, items = check_against_definition(w, full, [values[(p, k)] for k in range(w.D)])
        rows[pointer] = [items[offsets[k]:offsets[k + 1]] if valid[k] else None for k in range(w.D)]
    assert rows[""][:5] == [[], [[], []], [{}], [[1, 2], [3]], [{"a": [1, 2]}, 3]] and rows[""][5:] == [None] * 6
    assert rows["/a"][5] == [1, "x\n", None, True, 2.5, {"b": [7]}] and rows["/a"][10] == [[[]], [], {"a": []}]
    assert rows["/a"][:5] == [None] * 5 and rows["/a"][6:10] == [None] * 4
    assert rows["/a/b"][8] == [7] and [r for k, r in enumerate(rows["/a/b"]) if k != 8] == [None] * 10
    assert rows["/zz"] == [None] * 11
    # dropping the closer clause would count the ']' of [] as an element of [[],[]]
    assert atwin.acm_is_candidate(ord("["), ord("]")) == 0 and atwin.acm_is_candidate(ord(","), ord("}")) == 0
    assert atwin.acm_is_candidate(ord("["), ord("[")) == 1 and atwin.acm_is_candidate(ord(","), ord('"')) == 1
    assert atwin.acm_is_candidate(ord(":"), ord("1")) == 0 and atwin.acm_is_candidate(ord("1"), ord(",")) == 0


def test_invalid_documents_are_no_arrays(oracle, nm, vtwin, stwin, atwin):
    """One document of every verdict code between valid ones: its row is not valid, has no element and is in neither count."""
    valid = [doc for doc, _ in tvm.seeded_documents(20260, 64)]
    data, docs, bad = tdk.mixed_stream(valid)
    pointers = ["", "/a"] + tsm.draw_paths(random.Random(5), [d for k, d in enumerate(docs) if k not in bad])[1:8]
    w = tdm.WindowArrays(oracle, nm, data, is_final=True)
    verdicts, _ = tdm.twin_documents(vtwin, w, 3)
    assert all(verdicts[k][0] == c for k, c in bad.items())
    check_window(w, stwin, atwin, pointers, docs, verdicts=verdicts)


def test_cut_window_no_document_and_capacities(oracle, nm, stwin, atwin):
    """A cut last document has no row.  No complete document, no token: offsets[0] = 0 and a zero result.  capacity one short
    and 0: MSJ_CAPACITY, n_rows = D, nothing else written.  elements_capacity one short and 0: offsets and validity complete,
    the elements clipped, MSJ_CAPACITY, n_elements exact.  d_elements NULL: the layout alone, code 0."""
    docs = [b'{"a":[1,2,{"b":"x\\ny"}],"cut":1}', b"[1.5,true]", b'{"a":[]}', b'{"a":["s",[4]]}']
    w = tdm.WindowArrays(oracle, nm, b" ".join(docs) + b' {"a":[1,"abc', is_final=False)
    assert (w.docs[0], w.D) == (5, 4) and w.T < w.n
    got, values = column_values(w, stwin, ["/a"], docs, capacity=6)
    records = got.column(0)[:w.D].copy()
    vals = [values[(0, k)] for k in range(w.D)]
    full = twin_lists(atwin, w, records, capacity=6)
    offsets, _, items = check_against_definition(w, full, vals)
    assert offsets == [0, 3, 3, 3, 5] and items == [1, 2, {"b": "x\ny"}, "s", [4]]
    for data in (b'{"a":[1,"abc', b"  \n "):
        w0 = tdm.WindowArrays(oracle, nm, data, is_final=False)
        assert w0.D == 0
        for cap in (3, 0):
            none = twin_lists(atwin, w0, records[:0], capacity=cap, elements_capacity=2)
            assert none.summary() == (0,) * 10 + (1, 0, 0, 0) and none.untouched(0, 0) and (cap == 0 or none.offsets[0] == 0)
    for cap in (w.D - 1, 0):
        short = twin_lists(atwin, w, records, capacity=cap, elements_capacity=5)
        assert short.summary() == (MSJ_CAPACITY, 0, w.D, 0, 0, 0, 0, MSJ_CAPACITY, 0, 0, 1, 0, 0, 0) and short.untouched(-1, 0)
    for room in (4, 0, 2):
        clip = twin_lists(atwin, w, records, elements_capacity=room)
        assert clip.summary()[:7] == (MSJ_CAPACITY, 0, 4, 3, 5, 0, 0) and clip.summary()[7:] == (MSJ_CAPACITY, 0, 5, 1, 5, 0, 0)
        assert np.array_equal(clip.offsets, twin_lists(atwin, w, records, elements_capacity=5).offsets) and clip.untouched(w.D, room)
        assert np.array_equal(clip.elements[:room], full.elements[:room]) and np.array_equal(clip.valid[:w.D], full.valid[:w.D])
    layout = twin_lists(atwin, w, records, layout_only=True)
    assert layout.summary() == full.summary() and layout.res.code == 0 and layout.res.n_elements == 5


def test_numbers_without_records(oracle, nm, stwin, atwin):
    """d_numbers NULL, d_numbers_result NULL, or fewer records than an element's: MSJ_FIELD_NO_BITS, bits 0 and the right
    tag, counted only where written; the value comes from the text.  With the records: the bits."""
    docs = [b'{"v":[-12,1.5e2,"x",0.0]}', b'{"v":[3,[4.25],9223372036854775807]}', b'{"v":[-0,{"n":1}]}']
    w = tdm.WindowArrays(oracle, nm, tdk.join(docs, b"\n"), is_final=True)
    got, values = column_values(w, stwin, ["/v"], docs)
    records = got.column(0)[:w.D].copy()
    vals = [values[(0, k)] for k in range(w.D)]
    full = twin_lists(atwin, w, records)
    check_against_definition(w, full, vals)
    assert [chr(int(t)) for t in full.elements[:9]["type"]] == list('ld"dl[ll{') and int(full.elements[6]["bits"]) == (1 << 63) - 1
    for kw in (dict(numbers=False), dict(numbers_result=False)):
        part = twin_lists(atwin, w, records, **kw)
        check_against_definition(w, part, vals, bits=False)
        assert part.res.n_no_bits == 6
        for a, b in zip(part.elements[:9], full.elements[:9]):
            assert (a["type"], a["token"], a["code"]) == (b["type"], b["token"], b["code"])
            assert (int(a["bits"]), int(a["flags"])) == (0, _lib.FIELD_NO_BITS) if chr(int(b["type"])) in "ld" else a == b
    few = twin_lists(atwin, w, records, numbers_capacity=3)    # the first document's records only
    check_against_definition(w, few, vals, bits=False)
    assert few.res.n_no_bits == 3 and np.array_equal(few.elements[:4], full.elements[:4])
    clipped = twin_lists(atwin, w, records, numbers=False, elements_capacity=2)
    assert clipped.res.n_no_bits == 2 and clipped.res.code == MSJ_CAPACITY    # (only the records written count)


def test_select_result_is_cross_checked(oracle, nm, stwin, atwin):
    """A d_select with a code: that code, a zero result, nothing written.  One with another D: MSJ_ERR_BAD_ARGUMENT."""
    docs = [b"[1,2]", b"[3]"]
    w = tdm.WindowArrays(oracle, nm, tdk.join(docs, b"\n"), is_final=True)
    records = tsm.twin_select(stwin, w, [""]).column(0)[:w.D].copy()
    for code in (MSJ_CAPACITY, 7):
        got = twin_lists(atwin, w, records, sel_code=code, elements_capacity=3)
        assert got.summary() == (code, 0, 0, 0, 0, 0, 0, code, 0, 0, 1, 0, 0, 0) and got.untouched(-1, 0)
    for D in (1, 3, 0):
        got = twin_lists(atwin, w, records, sel_D=D, capacity=4, elements_capacity=3)
        assert got.summary() == (BAD_ARGUMENT, 0, 0, 0, 0, 0, 0, BAD_ARGUMENT, 0, 0, 1, 0, 0, 0) and got.untouched(-1, 0)


def hostile_records(w):
    """For the window of `hostile_window`: records no select call writes, each next to the good record of its row
    -> (records, the rows that stay arrays)"""
    n = w.n
    f = w.first[:w.D].tolist()
    recs = [record(f[0]),                      # good: [1,2]
            record(n),                         # token == n
            record(0xFFFFFFFF),                # the token of a record with a code, but code 0
            record(f[0]),                      # row 3 names document 0's array
            record(f[4] + 3),                  # good: the '[' of {"a":[6,7]}
            record(f[5]),                      # a '[' record on a '{' token
            record(f[6]),                      # good
            record(f[6], typ="{"),             # the right token, the wrong tag
            record(f[8], code=20),             # a code: in neither count
            record(f[9] + 1)]                  # the inner '[' of [[1],2]: a nested array is a row when the record names it
    return np.concatenate(recs), [0, 4, 6, 9]


HOSTILE = [b"[1,2]", b"[3]", b"[4]", b"[5]", b'{"a":[6,7]}', b'{"a":[8]}', b"[9,[10]]", b"[11]", b"[12]", b"[[1],2]"]


def test_hostile_records(oracle, nm, atwin):
    """token >= n, a token of another document, a '[' record on a '{' token, the wrong tag, a code: no array, nothing read
    out of bounds, no element.  A partner past e_k (the arrays edited): no array either."""
    w = tdm.WindowArrays(oracle, nm, tdk.join(HOSTILE, b"\n"), is_final=True)
    records, good = hostile_records(w)
    got = twin_lists(atwin, w, records)
    assert [k for k in range(w.D) if got.valid[k]] == good
    assert got.offsets[:w.D + 1].tolist() == [0, 2, 2, 2, 2, 4, 4, 6, 6, 6, 7] and got.res.n_other == 5 and got.res.n_arrays == 4
    data = np.frombuffer(w.data, dtype=np.uint8)
    assert [field_value(r, data, w.idx, w.end) for r in got.elements[:7]] == [1, 2, 6, 7, 9, [10], 1]
    # the partner of document 1's array moved to document 2's closing bracket, and to "no partner"
    f1 = int(w.first[1])
    for m in (int(w.first[2]) + 2, tdk.NO_PARTNER, f1, w.n + 5):
        w.match = w.match.copy()
        w.match[f1] = m
        got = twin_lists(atwin, w, np.concatenate([record(int(f)) for f in w.first[:w.D]]))
        assert got.valid[:3].tolist() == [1, 0, 1] and got.offsets[:4].tolist() == [0, 2, 2, 3]
    v, m, cd = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_int32()
    arrs = [np.ascontiguousarray(a) for a in (w.typ, w.depth, w.match)]
    row = lambda rec, ok, f, e: atwin.acm_row(rec.ctypes.data, ok, f, e, *[a.ctypes.data for a in arrs], ctypes.byref(v), ctypes.byref(m), ctypes.byref(cd))
    assert row(record(0), 1, 0, 5) == 1 and (v.value, m.value, cd.value) == (0, 4, 1)
    assert row(record(0), 0, 0, 5) == 2 and row(record(0), 1, 0, 4) == 2 and row(record(0), 1, 1, 5) == 2 and (v.value, m.value) == (0xFFFFFFFF, 0)
    assert row(record(0, code=17), 1, 0, 5) == 0
