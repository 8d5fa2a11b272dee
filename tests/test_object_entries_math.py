"""CPU check of msj_object_entries_device's arithmetic (mojo_simdjson_amd/csrc/object_entries_math.h).

The definition in include/msj_stage1.h is restated in Python from its text alone (`definition` below), on json with
object_pairs_hook=list, so that duplicate keys and their order are visible: a row that is an object gives its (key, value)
pairs, every other row is no object.  The rows come from all four sources the call names -- one path's column of the select
twin (the rows are the documents), the element records of the array-column twin, one path of the select-elements twin, and
this twin's own value records, two levels deep.  The host twin (tests/object_entries_math_host.cpp: the verdict on the rows,
the live rows, the order test, the row, candidate and entry tests of the headers with select_math.h's record, serially)
must give the definition's offsets and validity bytes; every key record decoded and unescaped and every value record
decoded through field_value must equal the definition's, fill and canary behind every array included.  Hostile records and
malformed members -- which json cannot describe -- are pinned by value.  The kernels that run the same headers on the device
are covered by tests/test_object_entries.py (-m gpu).
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
from tests import test_array_column_math as tac
from tests import test_array_elements_math as tae
from tests import test_number_math as tnm
from tests import test_select_elements_math as tse
from tests import test_select_math as tsm
from tests import test_tape_documents_math as tdk
from tests import test_validate_documents_math as tdm
from tests import test_validate_math as tvm

MSJ_CAPACITY, BAD_ARGUMENT = 1, -1
NO_TOKEN = 0xFFFFFFFF
NO_SUCH_FIELD, INCORRECT_TYPE = 20, 17

# the objects the definition is pinned on, each the value at /m of one document
PIN_OBJECTS = [b"{}", b'{"a":{"b":1,"c":{"d":2}},"e":[{"f":3}]}', b'{"a":"b"}', b'{"a":"b","c":"d"}',
               b'{"q\\"\\\\\\/\\b\\f\\n\\r\\t\\u00e9\\ud83d\\ude00":1,"\\u0041":2}', b'{"k":1,"k":2,"j":3,"k":{"k":4}}', b'{"":0,"x":""}',
               b'{"s":"v","e":"\\n","i":-7,"d":2.5e3,"t":true,"f":false,"n":null,"o":{},"a":[],"oo":{"x":1},"aa":[1,{"y":2}]}']
DEPTH_PIN = b'{"a":{"b":1}}'           # without the depth clause of the entry test "b" would be an entry of the row too
COLON_PIN = b'{"a":"b","c":1}'         # without the ':' clause of the candidate test "b" would be a key (its "value": "c")
PIN_TEXTS = [b'{"m":' + o + b"}" for o in PIN_OBJECTS] + [b'{"m":7}', b'{"x":{"m":{"a":1}}}', b'{"m":[{"a":1}]}', b'{"m":' + DEPTH_PIN + b"}",
                                                          b'{"m":' + COLON_PIN + b"}"]

_twins = {}


def load_twin(mutation=None):
    """The host twin of the call (g++ build of tests/object_entries_math_host.cpp); mutation: "DEPTH" the entry test without
    its depth clause, "COLON" the candidate test without its ':' clause."""
    if mutation in _twins:
        return _twins[mutation]
    os.makedirs(tvm.BUILD, exist_ok=True)
    so = os.path.join(tvm.BUILD, "libobject_entries_math_host%s.so" % ("_no_" + mutation.lower() if mutation else ""))
    src = os.path.join(helpers.ROOT, "tests", "object_entries_math_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared"] + (["-DMSJ_TWIN_NO_%s_CLAUSE" % mutation] if mutation else []) + ["-o", so, src])
    lib = ctypes.CDLL(so)
    vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32
    for name, args, res in (("oem_object_entries", [vp, u64] + [vp] * 6 + [u64, vp, vp, vp, vp, vp, u64, vp, vp, u64, vp, vp, vp], None),
                            ("oem_is_key_candidate", [u32, u32], ctypes.c_int), ("oem_is_entry_of", [u64, i32, u32, u32, i32], ctypes.c_int)):
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
    t.l, t.o = tae.load_twin(), load_twin()
    return t


# ---- the twin ---------------------------------------------------------------------------------------------------------------

class Maps:
    """What one call left: the three results and the four arrays, each with its fill and 64 bytes of canary behind its
    capacity.  keys and values are None in the layout-only form."""

    def __init__(self, res, ksel, vsel, offsets, valid, keys, values, capacity, entries_capacity):
        self.res, self.ksel, self.vsel, self.offsets, self.valid, self.keys, self.values = res, ksel, vsel, offsets, valid, keys, values
        self.capacity, self.entries_capacity = capacity, entries_capacity

    def summary(self):
        r = self.res
        sel = lambda e: (e.code, e.flags, e.n_documents, e.n_paths, e.n_found, e.n_no_bits, e.reserved)
        return (r.code, r.flags, r.n_rows, r.n_objects, r.n_entries, r.n_other, r.n_no_bits) + sel(self.ksel) + sel(self.vsel)

    def untouched(self, rows, n_entries):
        """Offsets past `rows` (-1: none written at all), validity bytes at or past it, key and value records at or past
        `n_entries`, and the canaries, are as they were filled"""
        ok = bool((self.offsets.view(np.uint8)[8 * (rows + 1):] == tac.FILL).all()) and bool((self.valid[max(rows, 0):] == tac.FILL).all())
        return ok and (self.keys is None or all(bool((a.view(np.uint8)[16 * n_entries:] == tac.FILL).all()) for a in (self.keys, self.values)))


def stop_summary(code, n_rows=0):
    """The three results of a call that stopped in front of the layout"""
    return (code, 0, n_rows, 0, 0, 0, 0) + (code, 0, 0, 1, 0, 0, 0) * 2


def twin_maps(otwin, w, rows, rows_select=None, capacity=None, entries_capacity=None, layout_only=False, numbers=True, numbers_result=True,
              numbers_capacity=None):
    """oem_object_entries over the window's arrays and the records `rows`.  rows_select None: a result for len(rows) rows.
    entries_capacity None: what a layout-only first call reports.  numbers False: d_numbers NULL with capacity 0;
    numbers_result False: d_numbers_result NULL.  -> Maps"""
    rows = np.ascontiguousarray(rows)
    rows_select = tse.rows_result(rows.size) if rows_select is None else rows_select
    capacity = max(rows.size, 1) if capacity is None else capacity
    kw = dict(rows_select=rows_select, capacity=capacity, numbers=numbers, numbers_result=numbers_result, numbers_capacity=numbers_capacity)
    if entries_capacity is None and not layout_only:
        entries_capacity = int(twin_maps(otwin, w, rows, layout_only=True, **kw).res.n_entries)
    room = 0 if layout_only else entries_capacity
    offsets, valid, keys = tac.filled(capacity, room, layout_only)
    values = None if layout_only else keys.copy()
    res, ksel, vsel = _lib.MsjObjectEntriesResult(), _lib.MsjSelectDocumentsResult(), _lib.MsjSelectDocumentsResult()
    ncap = (int(w.records.size) if numbers_capacity is None else numbers_capacity) if numbers else 0
    recs = np.ascontiguousarray(w.records[:ncap])
    nr = w.numbers_result()
    arrs = [np.ascontiguousarray(a) for a in (w.idx, w.typ, w.depth, w.match, w.end, w.flags)]
    otwin.oem_object_entries(arrs[0].ctypes.data, w.n, *[a.ctypes.data for a in arrs[1:]], recs.ctypes.data if ncap else None, ncap,
                             ctypes.byref(nr) if numbers_result else None, rows.ctypes.data if rows.size else None, ctypes.byref(rows_select),
                             offsets.ctypes.data, valid.ctypes.data, capacity, keys.ctypes.data if keys is not None else None,
                             values.ctypes.data if values is not None else None, room, ctypes.byref(res), ctypes.byref(ksel), ctypes.byref(vsel))
    return Maps(res, ksel, vsel, offsets, valid, keys, values, capacity, room)


def record(token, typ="{", bits=0, flags=0, code=0):
    return tac.record(token, typ, bits, flags, code)


def coded(code):
    """A record as the select calls write it for a lookup that failed"""
    return record(NO_TOKEN, typ="", code=code)


def document_rows(twins, w, pointer, verdicts=None):
    """Source 1: one path's column of the select twin, the rows are the documents -> (records, their result)"""
    got = tsm.twin_select(twins.s, w, [pointer], verdicts=verdicts)
    return got.column(0)[:w.D].copy(), got.res


def rows_of(twins, w, source, verdicts=None):
    """source: ("doc", pointer) | ("list", list_pointer) | ("sub", list_pointer, sub) -> (records, their result)"""
    if source[0] == "doc":
        return document_rows(twins, w, source[1], verdicts)
    return tae.parent_rows(twins, w, source[1], source[2] if source[0] == "sub" else None, verdicts=verdicts)


def next_level(maps):
    """A twin's complete output as the next call's rows: the value records"""
    return maps.values[:int(maps.res.n_entries)].copy(), maps.vsel


# ---- the definition ---------------------------------------------------------------------------------------------------------

class Pairs(list):
    """A JSON object as its (key, value) pairs in document order, duplicates kept"""


_DECODER = json.JSONDecoder(object_pairs_hook=Pairs)


def decode(text):
    return _DECODER.decode(text.decode("utf-8"))


def lookup(value, pointer):
    """A pointer of object keys in a decoded document, the FIRST of duplicate keys taken -> (code, value)"""
    for seg in [s.replace("~1", "/").replace("~0", "~") for s in pointer.split("/")[1:]]:
        if not isinstance(value, Pairs):
            return INCORRECT_TYPE, None
        hits = [v for k, v in value if k == seg]
        if not hits:
            return NO_SUCH_FIELD, None
        value = hits[0]
    return 0, value


def plain(value):
    """Pairs as the dict field_value decodes a container's text to: the first of duplicate keys wins"""
    if isinstance(value, Pairs):
        out = {}
        for k, v in value:
            out.setdefault(k, plain(v))
        return out
    return [plain(v) for v in value] if isinstance(value, list) else value


def definition_rows(texts, source, codes=None):
    """[(code, value) per row] of one source over the documents `texts`; codes: their verdict codes (None: all 0)"""
    rows = []
    for k, text in enumerate(texts):
        bad = codes[k] if codes and codes[k] else 0
        if source[0] == "doc":
            rows.append((bad, None) if bad else lookup(decode(text), source[1]))
            continue
        code, v = (bad, None) if bad else lookup(decode(text), source[1])
        if code == 0 and isinstance(v, list) and not isinstance(v, Pairs):
            rows += [(0, item) if source[0] == "list" else lookup(item, source[2]) for item in v]
    return rows


def definition(values):
    """values: (code, value) per row -> (offsets, valid, (key, value) pairs back to back, n_other)"""
    offsets, valid, pairs, n_other = [0], [], [], 0
    for code, v in values:
        is_object = code == 0 and isinstance(v, Pairs)
        valid.append(int(is_object))
        n_other += code == 0 and not is_object
        if is_object:
            pairs += list(v)
        offsets.append(len(pairs))
    return offsets, valid, pairs, n_other


def values_of(values):
    """The next level's rows: the values of the rows that are objects"""
    return [(0, v) for code, row in values if code == 0 and isinstance(row, Pairs) for _, v in row]


def check_against_definition(w, got, values, bits=True):
    """A twin's (or the device's) complete column -- room for every row and every entry -- against the definition"""
    offsets, valid, pairs, n_other = definition(values)
    R = len(values)
    assert got.offsets[:R + 1].tolist() == offsets and got.valid[:R].tolist() == valid
    data = np.frombuffer(w.data, dtype=np.uint8)
    no_bits = 0
    for j, (key, want) in enumerate(pairs):
        k, r = got.keys[j], got.values[j]
        assert (k["code"], chr(int(k["type"])), int(k["flags"]) & ~2) == (0, '"', 0) and k["token"] + 2 == r["token"], (j, k, r)
        assert field_value(k, data, w.idx, w.end) == key, (j, k, key)
        assert r["code"] == 0 and chr(int(r["type"])) in '{["ldtfn', (j, r)
        if bits:
            assert not r["flags"] & _lib.FIELD_NO_BITS, (j, r)
        no_bits += bool(r["flags"] & _lib.FIELD_NO_BITS)
        value = field_value(r, data, w.idx, w.end)
        assert tsm.same_value(value, plain(want)), (j, r, value, want)
    n = len(pairs)
    assert got.summary() == (0, 0, R, sum(valid), n, n_other, no_bits, 0, 0, n, 1, n, 0, 0, 0, 0, n, 1, n, no_bits, 0), got.summary()
    assert got.untouched(R, n)
    return offsets, valid, pairs


def check_window(oracle, nm, twins, texts, source, verdicts=False, sep=b"\n", levels=1):
    """One window the whole way: rows from the sibling twins, this twin in the layout-only form and complete, against the
    definition; levels > 1: the call over its own values -> (WindowArrays, rows, rows_select, the first level's Maps, values)"""
    w = tdm.WindowArrays(oracle, nm, tdk.join(texts, sep), is_final=True)
    assert w.D == len(texts)
    rows_v = tdm.twin_documents(twins.v, w, 100)[0] if verdicts else None
    rows, rsel = rows_of(twins, w, source, verdicts=rows_v)
    values = definition_rows(texts, source, [c for c, _ in rows_v] if rows_v else None)
    first = None
    for level in range(levels):
        assert rows.size == len(values), (source, level)
        full = twin_maps(twins.o, w, rows, rsel)
        check_against_definition(w, full, values)
        layout = twin_maps(twins.o, w, rows, rsel, layout_only=True)
        assert layout.summary() == full.summary() and layout.keys is None and layout.values is None
        assert np.array_equal(layout.offsets, full.offsets) and np.array_equal(layout.valid, full.valid)
        first = first or (w, rows, rsel, full, values)
        (rows, rsel), values = next_level(full), values_of(values)
    return first


# ---- a seeded corpus of maps, lists of maps, maps inside lists of structs and maps of maps -------------------------------------

KEYS = ["", "a", "color", "size", "2024-01-01", "k\n", "é\U0001F600", 'q"\\/', "x" * 40, "a/b", "~"]


def _scalar(rng):
    return rng.choice([rng.randrange(-1000, 1000), 0.5, -2.5e3, "", "plain", "e\nsc", "é\U0001F600", None, True, False])


def _map(rng, depth=0):
    out = Pairs()
    for _ in range(rng.randrange(5)):
        kind = rng.randrange(8 if depth < 3 else 4)
        key = rng.choice(KEYS)
        if kind < 4:
            out.append((key, _scalar(rng)))
        elif kind < 6:
            out.append((key, _map(rng, depth + 1)))
        elif kind == 6:
            out.append((key, [_scalar(rng), _map(rng, depth + 1), [Pairs([("in", 1)])]]))
        else:
            out.append((key, rng.choice([[], Pairs()])))
    return out


def dumps(value, **kw):
    """json.dumps that writes Pairs as an object with every pair, duplicates included"""
    if isinstance(value, Pairs):
        sep = kw.get("separators", (", ", ": "))
        return "{" + sep[0].join(json.dumps(k, ensure_ascii=kw.get("ensure_ascii", True)) + sep[1] + dumps(v, **kw) for k, v in value) + "}"
    if isinstance(value, list):
        return "[" + kw.get("separators", (", ", ": "))[0].join(dumps(v, **kw) for v in value) + "]"
    return json.dumps(value, **kw)


def _struct(rng):
    kind = rng.randrange(8)
    if kind == 0:
        return _scalar(rng)                          # an element that is no object: 17
    if kind == 1:
        return Pairs([("sku", _scalar(rng))])        # no dims: 20
    dims = _map(rng, 1) if kind < 6 else rng.choice([7, "t", [Pairs([("w", 1)])], None])
    return Pairs([("sku", _scalar(rng)), ("x", Pairs([("dims", Pairs([("deep", 0)]))])), ("dims", dims), ("after", [_scalar(rng)])])


def seeded_documents(seed, n_docs):
    """n_docs lines {"id": k, "attrs": {map}, "maps": [maps ...], "items": [structs with "dims" ...]} -- or something else at
    attrs / maps / items now and then; escaped and plain spellings, compact and spaced separators alternate"""
    rng = random.Random(seed)
    out = []
    for k in range(n_docs):
        attrs = _map(rng) if k % 9 else rng.choice([7, [Pairs([("a", 1)])], None, "s"])
        maps = [_map(rng) if rng.randrange(4) else _scalar(rng) for _ in range(rng.randrange(5))] if k % 7 else Pairs([("a", 1)])
        items = [_struct(rng) for _ in range(rng.randrange(6))] if k % 11 else rng.choice([7, Pairs([("dims", Pairs())])])
        doc = Pairs([("id", k), ("attrs", attrs), ("maps", maps), ("items", items)])
        out.append(dumps(doc, ensure_ascii=bool(k % 2), separators=(",", ":") if k % 3 else (", ", ": ")).encode("utf-8"))
    return out


SOURCES = (("doc", "/attrs"), ("list", "/maps"), ("sub", "/items", "/dims"), ("sub", "/items", ""), ("doc", ""))


# ---- tests ------------------------------------------------------------------------------------------------------------------

def test_corpus_equals_definition(oracle, nm, twins):
    """Seeded documents under the four separators, rows from the document column, from list elements and from a
    select-elements path, each followed two levels down through the call's own values: rows that are objects, other values
    and codes 17 and 20 alike."""
    objects = entries = coded_rows = 0
    for j, sep in enumerate((b"\n", b" ", b"\r\n", b"")):
        texts = seeded_documents(6100 + j, 100)
        for source in SOURCES:
            _, rows, _, full, values = check_window(oracle, nm, twins, texts, source, sep=sep, levels=3)
            objects, entries = objects + int(full.res.n_objects), entries + int(full.res.n_entries)
            coded_rows += sum(c != 0 for c, _ in values)
    assert objects > 1000 and entries > 2000 and coded_rows > 100, (objects, entries, coded_rows)


def test_pins(oracle, nm, twins):
    """The cases read from the definition: {}; nested objects whose inner keys are not the row's; a string value is no key;
    keys with every escape kind and a surrogate pair; duplicate keys, all kept in order; the empty key; values of every type;
    rows that are no object.  Then the two mutations, each shown to fail its pin."""
    w, rows, _, full, values = check_window(oracle, nm, twins, PIN_TEXTS, ("doc", "/m"))
    offsets, valid, pairs = definition(values)[:3]
    per_row = [[k for k, _ in pairs[offsets[r]:offsets[r + 1]]] if valid[r] else None for r in range(len(values))]
    assert per_row[:4] == [[], ["a", "e"], ["a"], ["a", "c"]]
    assert per_row[4] == ['q"\\/\b\f\n\r\té\U0001F600', "A"] and per_row[5] == ["k", "k", "j", "k"] and per_row[6] == ["", "x"]
    assert per_row[7] == ["s", "e", "i", "d", "t", "f", "n", "o", "a", "oo", "aa"]
    assert per_row[8:] == [None, None, None, ["a"], ["a", "c"]]    # (20 at /m of {"x":...}: a code, no row)
    assert [v for _, v in pairs[offsets[5]:offsets[6]]] == [1, 2, 3, Pairs([("k", 4)])]
    assert [chr(int(t)) for t in full.values[offsets[7]:offsets[8]]["type"]] == list('""ldtfn{[{[')
    assert full.keys[offsets[4]]["flags"] == 2 and full.keys[offsets[3]]["flags"] == 0          # MSJ_SPAN_ESCAPED on the key's record
    assert (full.res.n_objects, full.res.n_other, full.res.n_rows) == (10, 2, 13)
    # the value of an entry two levels down: the call over its own values sees the inner objects only
    deep = twin_maps(twins.o, w, *next_level(full))
    assert deep.res.n_objects == 5 and deep.res.n_entries == 2 + 1 + 1 + 0 + 1
    for pin, mutation, right, wrong in ((DEPTH_PIN, "DEPTH", 1, 2), (COLON_PIN, "COLON", 2, 3)):
        alone = tdm.WindowArrays(oracle, nm, pin + b"\n", is_final=True)
        r1, s1 = document_rows(twins, alone, "")
        assert int(twin_maps(twins.o, alone, r1, s1).res.n_entries) == right
        assert int(twin_maps(load_twin(mutation), alone, r1, s1).res.n_entries) == wrong
    # ({"a":"b"} alone cannot show the ':' mutation: its "b" has no token i + 2 in front of the '}', so the value clause
    # already keeps it out; the pin adds a member behind it)
    t = twins.o
    assert t.oem_is_key_candidate(ord('"'), ord(":")) and not t.oem_is_key_candidate(ord('"'), ord(",")) and not t.oem_is_key_candidate(ord("{"), ord(":"))
    assert t.oem_is_entry_of(5, 3, 4, 8, 3) and not t.oem_is_entry_of(6, 3, 4, 8, 3) and not t.oem_is_entry_of(4, 3, 4, 8, 3)
    assert not t.oem_is_entry_of(5, 4, 4, 8, 3)


def test_rows_in_documents_with_verdict_codes(oracle, nm, twins):
    """Documents with a verdict code between valid ones: as document rows they carry the code and have no entries; as lists
    they are no rows of the parent column."""
    texts = [b'{"m":{"a":1},"l":[{"b":2}]}', b'{"m":{"a":tru},"l":[{"b":2}]}', b'{"m":{"c":3,"d":4},"l":[]}', b'{"m":{"e":5},,"l":[{"x":1}]}',
             b'{"m":{},"l":[{"f":6},{"g":7,"h":8}]}']
    _, rows, _, full, values = check_window(oracle, nm, twins, texts, ("doc", "/m"), verdicts=True)
    assert [c != 0 for c, _ in values] == [False, True, False, True, False] and full.offsets[:6].tolist() == [0, 1, 1, 3, 3, 3]
    _, rows, _, full, _ = check_window(oracle, nm, twins, texts, ("list", "/l"), verdicts=True)
    assert rows.size == 3 and full.offsets[:4].tolist() == [0, 1, 2, 4]


def test_numbers_without_records(oracle, nm, twins):
    """d_numbers NULL, d_numbers_result NULL, or fewer records than a value's: MSJ_FIELD_NO_BITS, bits 0 and the right tag,
    counted in the result and the values' select result only, and only where written."""
    texts = [b'{"m":{"a":-12,"b":1.5e2,"c":"x","d":0.0}}', b'{"m":{"e":3,"f":[4.25],"g":9223372036854775807,"h":{"n":1}}}']
    w, rows, rsel, full, values = check_window(oracle, nm, twins, texts, ("doc", "/m"))
    assert [chr(int(t)) for t in full.values[:8]["type"]] == list('ld"dl[l{') and int(full.values[6]["bits"]) == (1 << 63) - 1
    for kw in (dict(numbers=False), dict(numbers_result=False), dict(numbers_capacity=0)):
        part = twin_maps(twins.o, w, rows, rsel, **kw)
        check_against_definition(w, part, values, bits=False)
        assert part.res.n_no_bits == 5 and part.vsel.n_no_bits == 5 and part.ksel.n_no_bits == 0
        assert np.array_equal(part.keys, full.keys)
        for a, b in zip(part.values[:8], full.values[:8]):
            assert (a["type"], a["token"], a["code"]) == (b["type"], b["token"], b["code"])
            assert (int(a["bits"]), int(a["flags"])) == (0, _lib.FIELD_NO_BITS) if chr(int(b["type"])) in "ld" else a == b
    few = twin_maps(twins.o, w, rows, rsel, numbers_capacity=3)    # the first row's records only
    check_against_definition(w, few, values, bits=False)
    assert few.res.n_no_bits == 2 and np.array_equal(few.values[:4], full.values[:4])
    clipped = twin_maps(twins.o, w, rows, rsel, numbers=False, entries_capacity=2)
    assert clipped.res.n_no_bits == 2 and clipped.res.code == MSJ_CAPACITY and clipped.vsel.n_no_bits == 2    # (only the records written count)


def test_head_codes_and_capacities(oracle, nm, twins):
    """d_rows_select with a code: a zero result with that code.  R > capacity: MSJ_CAPACITY, n_rows = R.  R == 0 and n == 0:
    offsets[0] = 0 and a zero result.  entries_capacity short: offsets and validity complete, the records clipped, n_entries
    exact."""
    texts = [b'{"l":[{"a":1,"b":2},{"c":3},{}]}', b'{"l":[{"d":4,"e":{"f":5}}]}']
    w = tdm.WindowArrays(oracle, nm, tdk.join(texts, b"\n"), is_final=True)
    rows, esel = rows_of(twins, w, ("list", "/l"))
    for sel in (tse.rows_result(4, 9), tse.rows_result(4, -1), tse.rows_result(4, MSJ_CAPACITY)):
        got = twin_maps(twins.o, w, rows, sel, capacity=6, entries_capacity=8)
        assert got.summary() == stop_summary(sel.code) and got.untouched(-1, 0)
    for cap in (3, 0):
        got = twin_maps(twins.o, w, rows, esel, capacity=cap, entries_capacity=8)
        assert got.summary() == stop_summary(MSJ_CAPACITY, 4) and got.untouched(-1, 0)
    full = twin_maps(twins.o, w, rows, esel, capacity=6)
    assert full.summary()[:7] == (0, 0, 4, 4, 5, 0, 0) and full.offsets[:5].tolist() == [0, 2, 3, 3, 5] and full.untouched(4, 5)
    for room in (4, 0, 1):
        clip = twin_maps(twins.o, w, rows, esel, capacity=6, entries_capacity=room)
        assert clip.summary() == (MSJ_CAPACITY, 0, 4, 4, 5, 0, 0) + (MSJ_CAPACITY, 0, 5, 1, 5, 0, 0) * 2 and clip.untouched(4, room)
        assert np.array_equal(clip.offsets, full.offsets) and np.array_equal(clip.valid, full.valid)
        assert np.array_equal(clip.keys[:room], full.keys[:room]) and np.array_equal(clip.values[:room], full.values[:room])
    for cap in (3, 0):
        none = twin_maps(twins.o, w, rows[:0], capacity=cap, entries_capacity=2)
        assert none.summary() == stop_summary(0) and none.untouched(0, 0) and (cap == 0 or none.offsets[0] == 0)
    w0 = tdm.WindowArrays(oracle, nm, b"  \n ", is_final=True)
    assert w0.n == 0
    empty = twin_maps(twins.o, w0, rows[:0], capacity=2, entries_capacity=2)
    assert empty.summary() == stop_summary(0) and empty.offsets[0] == 0 and empty.untouched(0, 0)
    lost = twin_maps(twins.o, w0, rows, capacity=5, entries_capacity=2)   # records of another window over no token at all
    assert lost.summary()[:7] == (0, 0, 4, 0, 0, 4, 0) and lost.offsets[:5].tolist() == [0] * 5 and lost.valid[:4].tolist() == [0] * 4


# ---- hostile records ----------------------------------------------------------------------------------------------------------

#            0 1   2 3 4 5   6 7 8   9 10 11  12 13 14 15  16 17 18 19  20   21 22  23 24 25 26
HOSTILE = b'{ "a" : { "b" : 1 , "c" : {  "d" :  2  }  }  ,  "e" :  3  }  \n  {  "f" :  {  "g" :  4   }  } \n'
OUTER, FIRST, INNER, OTHER, LAST = 0, 3, 10, 21, 24   # the '{' tokens; n = 30


def hostile_window(oracle, nm):
    w = tdm.WindowArrays(oracle, nm, HOSTILE, is_final=True)
    assert w.n == 30 and [v for v in range(w.n) if w.typ[v] == ord("{")] == [OUTER, FIRST, INNER, OTHER, LAST]
    return w


def keys_per_row(got):
    """The key tokens of every valid row, None for the others"""
    R = int(got.res.n_rows)
    off = got.offsets[:R + 1].tolist()
    assert np.array_equal(got.keys[:off[R]]["token"] + 2, got.values[:off[R]]["token"])
    return [got.keys[off[r]:off[r + 1]]["token"].tolist() if got.valid[r] else None for r in range(R)]


def test_order_violations(oracle, nm, twins):
    """A descending or equal pair of live rows anywhere, also with coded rows between them: MSJ_ERR_BAD_ARGUMENT, n_rows = R,
    every count 0, only the results written.  Coded rows anywhere between ascending live rows: fine."""
    w = hostile_window(oracle, nm)
    good = [record(FIRST), record(INNER), record(OTHER), record(LAST)]
    assert keys_per_row(twin_maps(twins.o, w, np.concatenate(good))) == [[4, 8], [11], [22], [25]]
    for order in ([1, 0, 2, 3], [0, 1, 3, 2], [0, 2, 1, 3], [3, 0, 1, 2], [0, 1, 2, 2], [0, 0, 1, 2]):
        for gap in ([], [coded(20)], [coded(17), coded(20), coded(20)]):
            rows = []
            for j in order:
                rows += [good[j]] + gap
            rows = np.concatenate(gap + rows)
            got = twin_maps(twins.o, w, rows, entries_capacity=8)
            assert got.summary() == stop_summary(BAD_ARGUMENT, rows.size) and got.untouched(-1, 0), (order, len(gap))
    for gap in ([coded(20)], [coded(17), coded(20), coded(20)]):
        rows = []
        for g in good:
            rows += gap + [g] + gap
        got = twin_maps(twins.o, w, np.concatenate(rows))
        assert [t for t in keys_per_row(got) if t is not None] == [[4, 8], [11], [22], [25]] and got.res.code == 0
    tail = np.concatenate(good + [record(NO_TOKEN), coded(20)])      # a LIVE 0xFFFFFFFF can only be the last live row
    assert twin_maps(twins.o, w, tail).summary()[:7] == (0, 0, 6, 4, 5, 1, 0)
    assert twin_maps(twins.o, w, np.concatenate([record(NO_TOKEN)] + good), entries_capacity=8).res.code == BAD_ARGUMENT


def test_records_that_lie(oracle, nm, twins):
    """token >= n; a '{' record on a token that is none; a record of another type on a real object; a row whose own token is a
    key; a partner out of range or moved: no object, no entry, nothing read out of bounds -- and the row still owns its tokens."""
    w = hostile_window(oracle, nm)
    lying = np.concatenate([record(OUTER, typ="["), record(FIRST), record(5), record(8), record(INNER, typ='"'), coded(17), record(OTHER + 1),
                            record(w.n), record(w.n + 7), record(NO_TOKEN)])
    got = twin_maps(twins.o, w, lying)
    # (token 4 is the row FIRST's; the row at 5 owns 6..8, the row at 8 -- a key -- the rest up to INNER: neither is an object)
    assert keys_per_row(got) == [None, [4], None, None, None, None, None, None, None, None]
    assert got.offsets[:11].tolist() == [0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1] and (got.res.n_objects, got.res.n_other) == (1, 8)
    assert got.untouched(10, 1)
    # a row whose own token is a key of the row in front of it: counted in front of the row
    own = twin_maps(twins.o, w, np.concatenate([record(FIRST), record(8)]))
    assert keys_per_row(own) == [[4, 8], None] and own.offsets[:3].tolist() == [0, 2, 2]
    rows = np.concatenate([record(FIRST), record(INNER), record(OTHER)])
    for m in (w.n, w.n + 5, tdk.NO_PARTNER, INNER, INNER - 1, 0):
        w.match = w.match.copy()
        w.match[INNER] = m
        got = twin_maps(twins.o, w, rows)
        assert keys_per_row(got) == [[4, 8], None, [22]] and got.res.n_other == 1, m
    # a partner moved INSIDE the window: the row ends there, and a key needs its value in front of it
    for m, want in ((w.n - 1, [11]), (14, [11]), (13, []), (12, []), (11, [])):
        w.match[INNER] = m
        assert keys_per_row(twin_maps(twins.o, w, record(INNER))) == [want], m   # (no later key sits on the level of INNER's members)
    w.match[INNER], w.match[OUTER] = 14, 22    # ... and the outer object ending inside the second document: "f" is on no level of its
    assert keys_per_row(twin_maps(twins.o, w, record(OUTER))) == [[1, 17]]
    w.match[OUTER] = 19                        # "e" at 17 has its value at 19: not in front of the partner
    assert keys_per_row(twin_maps(twins.o, w, record(OUTER))) == [[1]]


def test_row_inside_a_row(oracle, nm, twins):
    """Ascending tokens with one row inside another: a token belongs to the LAST live row below it, and to that row alone."""
    w = hostile_window(oracle, nm)
    assert keys_per_row(twin_maps(twins.o, w, record(OUTER))) == [[1, 17]]
    nested = twin_maps(twins.o, w, np.concatenate([record(OUTER), record(FIRST)]))
    assert keys_per_row(nested) == [[1], [4, 8]] and nested.offsets[:3].tolist() == [0, 1, 3]    # 17 is nobody's
    assert keys_per_row(twin_maps(twins.o, w, np.concatenate([record(OUTER), coded(20), record(FIRST)]))) == [[1], None, [4, 8]]
    assert keys_per_row(twin_maps(twins.o, w, np.concatenate([record(OUTER), record(2)]))) == [[1], None]


def every_token_a_row(n_objects=600):
    """A window of {"k":j} objects inside one array, more than two blocks of tokens long"""
    return b"[" + b",".join(b'{"k":%d}' % j if j % 3 else b"{}" for j in range(n_objects)) + b"]\n"


def test_every_token_a_row(oracle, nm, twins):
    """Every token of the window is a row, each record claiming an object: a row owns the one token behind it, so the real
    objects keep their first entry, and the rest are no objects."""
    w = tdm.WindowArrays(oracle, nm, every_token_a_row(), is_final=True)
    assert w.n > 2048 + 64
    rows = np.concatenate([record(v) for v in range(w.n)])
    got = twin_maps(twins.o, w, rows)
    want = [[v + 1] if w.typ[v] == ord("{") and w.typ[v + 1] != ord("}") else ([] if w.typ[v] == ord("{") else None) for v in range(w.n)]
    assert keys_per_row(got) == want and got.res.n_objects == 600 and got.res.n_entries == 400
    assert got.untouched(w.n, 400)


MALFORMED = [(b'{"a":}', []), (b'{"a":,"b":1}', [(1, ","), (4, "l")]), (b'{"a" "b":1}', [(2, "l")]), (b'{"a":1 "b":2,:3}', [(1, "l"), (4, "l")])]


def malformed_rows(w):
    """A record for every '{' of the window, as a hostile caller would write them"""
    return np.concatenate([record(v) for v in range(w.n) if w.typ[v] == ord("{")])


def test_malformed_members(oracle, nm, twins):
    """Members that are no members, pinned by value: {"a":} has no token i + 2 in front of its '}'; a ',' or a key where the
    value should be is recorded as what it is.  And a key among the last three tokens of a cut window: its object has no
    partner, or -- with the partner moved to the window's last token -- no room for a value."""
    for text, want in MALFORMED:
        w = tdm.WindowArrays(oracle, nm, text + b"\n", is_final=True)
        got = twin_maps(twins.o, w, malformed_rows(w))
        assert [(int(k["token"]), chr(int(v["type"]))) for k, v in zip(got.keys[:len(want)], got.values[:len(want)])] == want, text
        assert got.res.n_entries == len(want) and got.res.code == 0
    w = tdm.WindowArrays(oracle, nm, b'{"z":0}\n{"a":1,"b":2,"c":3', is_final=False)
    n = w.n
    assert n == 5 + 12 and w.typ[n - 3] == ord('"') and w.match[5] == tdk.NO_PARTNER
    cut = twin_maps(twins.o, w, malformed_rows(w))
    assert keys_per_row(cut) == [[1], None] and cut.res.n_other == 1
    w.match = w.match.copy()
    w.match[5] = n - 1      # (hostile: the last token as the partner)
    moved = twin_maps(twins.o, w, malformed_rows(w))
    assert keys_per_row(moved) == [[1], [6, 10]]   # "c" at n - 3 has its value at n - 1: not in front of the partner
