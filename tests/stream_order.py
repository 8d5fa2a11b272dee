"""The corpus and the expected values of tests/test_stream_order.py: three NDJSON windows and, for each, what every call
of the chain behind stage 1 leaves in its output arrays -- from the oracles and the host twins alone, never from a device.

The chain: shard, stage2_prep(match), documents, number_values, validate_documents, tape_documents, select_documents over
POINTERS, string_column(/status), array_column(/items), select_elements over ELEMENT_POINTERS, array_elements(/items[*].tags),
object_entries(/attrs), raw_column(/geo) verbatim and compact, dictionary over the string column and over the compact raw
column.  Every capacity is fixed here, from the twins: the device test never sizes anything from a first call.

Window A holds the pieces that reach the device-only paths (ESCAPED_1K ... MISSING below); window B, the decoy, is A's lines in reversed order
with every value replaced by another of the same width, so that the byte length, the token count, the document count and
the number count are A's and every array differs; window C is a smaller, unrelated window.
"""
import functools
import json

import numpy as np

from mojo_simdjson_amd import _lib
from tests import helpers
from tests import test_array_column_math as tac
from tests import test_array_elements_math as tae
from tests import test_dictionary_math as tdc
from tests import test_number_math as tnm
from tests import test_object_entries_math as tom
from tests import test_raw_column_math as trm
from tests import test_select_elements_math as tse
from tests import test_select_math as tsm
from tests import test_string_column_math as tcm
from tests import test_tape_documents_math as tdk
from tests import test_tape_math as ttm
from tests import test_validate_documents_math as tdm

POINTERS = ["", "/status", "/tags", "/attrs", "/items", "/geo"]
P_STATUS, P_ATTRS, P_ITEMS, P_GEO = 1, 3, 4, 5
ELEMENT_POINTERS = ["/sku", "/q", "/tags", "/dims"]
E_TAGS = 2
ROOM = 3                 # rows of capacity past the rows a window has: the calls read the row count on the device
SENTINEL = 0x5A          # the byte of tests/test_validate_documents.py: SENTINEL
A_DOCS, C_DOCS = 600, 300
STATUS = ["active", "suspended", "closed", "", "actíve"]

# where window A's special documents are, by number
ESCAPED_1K, ESCAPED_4K = (5, 205, 405), 300      # escaped bodies over 1 024 and over 4 096 bytes (the waves' walks)
EQUAL_LONG, OTHER_LONG = (10, 310), 450          # strings of 600 bytes: two equal, one different (the dictionary's wave rows)
LONG_NUMBER, LONG_RAW, INVALID, MISSING = 20, 30, 7, 11

_SWAP = str.maketrans("abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789",
                      "bcdefghijklmnopqrstuvwxyzaBCDEFGHIJKLMNOPQRSTUVWXYZA0234567891")


def other(v):
    """The decoy's value for `v`: letters and digits changed one for one, the width and the kind kept; keys stay"""
    if isinstance(v, bool) or v is None:
        return v
    if isinstance(v, str):
        return v.translate(_SWAP)
    if isinstance(v, int):
        return int(str(v).translate(_SWAP))
    if isinstance(v, float):
        return float(repr(v).translate(_SWAP))
    if isinstance(v, list):
        return [other(x) for x in v]
    return {key: other(x) for key, x in v.items()}


def escaped(k, n):
    """A string whose JSON text has more than n bytes, most of them escapes, different for every k"""
    unit = "a\tb\"c\\dé%d\n" % k
    return unit * (n // 14 + 1)


def document_a(k):
    doc = {"id": k, "status": STATUS[(k * k) % 5], "tags": ["t%d" % (k % 4), k, "t%d" % (k % 3)],
           "attrs": {"color": "c%d" % (k % 3), "n%d" % (k % 6): k},
           "items": [{"sku": "s%d" % ((k + j) % 4), "q": j, "tags": ["u%d" % j, k % 7][:(k + j) % 3], "dims": {"w": j + 0.5, "h": [k % 5]}}
                     for j in range(k % 3 if k % 2 else 0)],
           "geo": {"lat": (k // 2) % 2, "lon": [k % 3]}}
    if k in ESCAPED_1K:
        doc["status"] = escaped(k, 1024)
    if k == ESCAPED_4K:
        doc["status"] = escaped(k, 4096)
    if k in EQUAL_LONG:
        doc["status"] = "long value " * 54 + "same  "
    if k == OTHER_LONG:
        doc["status"] = "long value " * 54 + "other "
    if k == LONG_NUMBER:
        doc["tags"][1] = "@@@@"   # (lines_a puts the number there)
    if k == LONG_RAW:
        doc["geo"]["note"] = "y" * 16500
    if k == MISSING:
        doc = {"id": k, "status": "active"}
    return doc


def document_c(k):
    doc = {"id": 3 * k, "status": ["new", "old", "n\new"][k % 3], "tags": [k % 2, "z"], "attrs": {"a": {"b": k}, "c": None},
           "items": [{"sku": k, "q": 1.5, "tags": [], "dims": {"d": "x%d" % k}}] * (k % 2), "geo": {"lat": -0.5, "lon": [1, 2, k]}}
    if k == 40:
        doc["status"] = escaped(k, 1100)
    if k % 50 == 49:
        del doc["items"]
    return doc


def line(k, doc, decoy=False):
    """Document k's text: pretty-printed every other line; the decoy's has the decoy's values in the same layout"""
    if decoy:
        doc = other(doc)
    return json.dumps(doc, indent=4 if k % 2 == 0 else None, separators=None if k % 2 == 0 else (",", ":")).encode()


def lines_a(decoy=False):
    out = [line(k, document_a(k), decoy) for k in range(A_DOCS)]
    number = "0." + "1234567890" * 7                       # a number of 72 characters
    bad = b'{"id":7,"status":"bad","tags":[tru]}'          # a verdict code: T_ATOM
    if decoy:
        number, bad = number.translate(_SWAP), b'{"id":8,"status":"cbe","tags":[tru]}'
    out[LONG_NUMBER] = out[LONG_NUMBER].replace(b'"@@@@"', number.encode())
    out[INVALID] = bad
    return out[::-1] if decoy else out


def lines_c():
    return [line(k + 1, document_c(k)) for k in range(C_DOCS)]


@functools.lru_cache(maxsize=None)
def corpus():
    """-> {"A" | "B" | "C": (the window's bytes, its lines)}"""
    return {name: (tdk.join(lines, b"\n"), lines) for name, lines in (("A", lines_a()), ("B", lines_a(decoy=True)), ("C", lines_c()))}


@functools.lru_cache(maxsize=None)
def twins():
    """Every host twin the chain has, and the oracles"""
    t = tse.Twins()
    t.l, t.o, t.c, t.r, t.d = tae.load_twin(), tom.load_twin(), tcm.load_twin(), trm.load_twin(), tdc.load_twin()
    t.tape, t.tm = tdk.load_twin(), ttm.load_twin()
    t.oracle, t.nm = helpers.load_oracle(), tnm.load_twin()
    return t


class Out:
    """One output array of one call: the expected bytes (fill and canary included), the byte it is filled with in front
    of the call, and how it is compared -- whole (upto None), only its first `upto` bytes (what lies behind them is not
    specified), or, a result struct, field by field (fields: those compared; None: all)."""

    def __init__(self, name, want, fill=tcm.FILL, upto=None, struct=None, fields=None):
        if struct is not None:
            want = np.frombuffer(bytes(want), dtype=np.uint8)
        self.name, self.fill, self.upto, self.struct = name, fill, upto, struct
        self.want = np.ascontiguousarray(want).view(np.uint8).reshape(-1).copy()
        self.fields = fields if fields is not None or struct is None else [f for f, _ in struct._fields_]

    def values(self, raw):
        """What is compared of `raw` (uint8, the array's size): a tuple of field values, or the bytes"""
        if self.struct is not None:
            s = self.struct.from_buffer_copy(raw.tobytes())
            return tuple(getattr(s, f) for f in self.fields)
        return raw[:self.upto]


def padded(a, n_bytes, fill=tcm.FILL):
    """The bytes of `a` with `n_bytes` of fill behind them: an array the call writes from its start, its canary behind it"""
    return np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.full(n_bytes, fill, dtype=np.uint8)])


def dictionary_of(t, col, rows, D):
    """The twin's dictionary of the first D rows of a twin's column (tcm.Column / trm.Column) of `rows` rows of capacity"""
    total = int(col.res.total_bytes)
    return tdc.twin_dictionary(t.d, tdc.Column(col.offsets[:rows + 1], col.valid[:rows], col.data[:total]), n_rows=D)


class Expected:
    """One window through the whole chain on the host.  calls: {call: [Out]} in the order of the chain."""

    def __init__(self, name, lines=None):
        t = twins()
        self.name = name
        self.data, self.lines = corpus()[name] if lines is None else (tdk.join(lines, b"\n"), list(lines))
        data, self.length = self.data, len(self.data)
        w = self.w = tdm.WindowArrays(t.oracle, t.nm, data, is_final=False)
        self.n, self.D, self.ncap = w.n, w.D, int(w.records.size)
        _, _, (final, lo, hi) = helpers.oracle_tokens(data, w.idx)
        opening = int(np.isin(w.typ, np.frombuffer(b"[{", dtype=np.uint8)).sum())   # (msj_tokens_result.reserved, include/msj_stage1.h)
        self.tokens = _lib.MsjTokensResult(w.n, final, lo, hi, opening)
        self.verdicts, self.vres = tdm.twin_documents(t.v, w, 100)
        self.codes = [c for c, _ in self.verdicts]
        self.tape = tdk.twin_window(t.tape, w, verdicts=self.verdicts, canary=8)
        rows = self.rows = w.D + ROOM
        self.sel = tsm.twin_select(t.s, w, POINTERS, verdicts=self.verdicts, capacity=rows)
        self.strings = tcm.twin_column(t.c, data, self.sel.column(P_STATUS), w.D, capacity=rows)
        self.lists = tac.twin_lists(t.a, w, self.sel.column(P_ITEMS), capacity=rows)
        self.E = int(self.lists.res.n_elements)
        erows = self.erows = self.E + ROOM
        self.efields = tse.twin_elements(t, w, ELEMENT_POINTERS, self.lists.elements, rows_select=self.lists.esel, capacity=erows)
        self.sublists = tae.twin_lists(t.l, w, self.efields.column(E_TAGS), rows_select=self.efields.res, capacity=erows)
        self.maps = tom.twin_maps(t.o, w, self.sel.column(P_ATTRS), rows_select=self.sel.res, capacity=rows)
        arrays = trm.arrays_of(w)
        self.raw = {c: trm.twin_raw(t.r, arrays, self.sel.column(P_GEO), R=w.D, compact=c, capacity=rows) for c in (False, True)}
        self.dict_strings = dictionary_of(t, self.strings, rows, w.D)
        self.dict_raw = dictionary_of(t, self.raw[True], rows, w.D)
        self.calls = self._calls()

    def _calls(self):
        w, S = self.w, _lib
        struct = lambda name, res, typ, fields=None: Out(name, res, struct=typ, fields=fields)
        column = lambda c, typ: [Out("offsets", c.offsets), Out("valid", c.valid), Out("data", c.data), struct("res", c.res, typ)]
        lists = lambda c: [Out("offsets", c.offsets), Out("valid", c.valid), Out("elements", c.elements), struct("res", c.res, S.MsjArrayColumnResult),
                           struct("esel", c.esel, S.MsjSelectDocumentsResult)]
        encoded = lambda e: [Out("codes", e.codes), Out("dict_offsets", e.dict_offsets), Out("dict_first", e.dict_first), Out("dict_bytes", e.dict_bytes),
                             struct("res", e.res, S.MsjDictionaryResult, ["code", "flags", "n_rows", "n_values", "n_distinct", "dict_bytes"])]
        selected = lambda s: [Out("fields", s.fields), struct("res", s.res, S.MsjSelectDocumentsResult)]
        carry = S.MsjCarry()
        carry.count = w.n
        m = self.maps
        return {
            # (behind the n indices stage 1 writes a trailer and nothing that a caller may read: the first n are compared)
            "shard": [Out("idx", padded(w.idx, 4 * (self.length + 7 - w.n)), upto=4 * w.n),
                      struct("carry", carry, S.MsjCarry, ["count", "in_string", "unescaped_error", "internal_error"])],
            "stage2_prep": [Out("type", padded(w.typ, 64)), Out("depth", padded(w.depth, 64)), Out("match", padded(w.match, 64)),
                            Out("end", padded(w.end, 64)), Out("flags", padded(w.flags, 64)), struct("res", self.tokens, S.MsjTokensResult)],
            "documents": [Out("first", padded(w.first[:w.D], 4 * ROOM + 64)), struct("res", S.MsjDocumentsResult(*w.docs), S.MsjDocumentsResult)],
            # (n_slow counts a path the kernel took: no twin has it)
            "number_values": [Out("records", padded(w.records, 64)),
                              struct("res", w.numbers_result(), S.MsjNumbersResult, ["n_numbers", "n_errors", "first_error"])],
            "validate_documents": [Out("rows", padded(tdk.verdict_rows(self.verdicts)[:w.D], 8 * 16, SENTINEL), SENTINEL),
                                   struct("res", self.vres, S.MsjValidateDocumentsResult)],
            "tape_documents": [Out("tape", self.tape.tape, tdk.BYTE_FILL), Out("sbuf", self.tape.sbuf, tdk.BYTE_FILL),
                               Out("recs", self.tape.recs, tdk.REC_FILL), struct("res", self.tape.res, S.MsjTapeDocumentsResult)],
            "select_documents": selected(self.sel),
            "string_column": column(self.strings, S.MsjStringColumnResult),
            "array_column": lists(self.lists),
            "select_elements": selected(self.efields),
            "array_elements": lists(self.sublists),
            "object_entries": [Out("offsets", m.offsets), Out("valid", m.valid), Out("keys", m.keys), Out("values", m.values),
                               struct("res", m.res, S.MsjObjectEntriesResult), struct("ksel", m.ksel, S.MsjSelectDocumentsResult),
                               struct("vsel", m.vsel, S.MsjSelectDocumentsResult)],
            "raw_column": column(self.raw[False], S.MsjRawColumnResult),
            "raw_column_compact": column(self.raw[True], S.MsjRawColumnResult),
            "dictionary_strings": encoded(self.dict_strings),
            "dictionary_raw": encoded(self.dict_raw),
        }

    def max_probe_holds(self, call, longest):
        """The bounds of tests/test_dictionary.py: same"""
        res = (self.dict_strings if call == "dictionary_strings" else self.dict_raw).res
        return (longest == 0) == (res.max_probe == 0) and longest <= max(tdc.MIN_SLOTS, 4 * int(res.n_rows))


    @classmethod
    def from_lines(cls, name, lines):
        """A window of the caller's own lines (tests/stale_tails.py) through the same chain"""
        return cls(name, lines)


@functools.lru_cache(maxsize=None)
def expected(name):
    return Expected(name)


def differing(x, y):
    """{call: the arrays of the call whose compared values differ between the windows x and y}"""
    out = {}
    for call in x.calls:
        out[call] = [a.name for a, b in zip(x.calls[call], y.calls[call])
                     if a.want.size != b.want.size or not np.array_equal(a.values(a.want), b.values(b.want))]
    return out
