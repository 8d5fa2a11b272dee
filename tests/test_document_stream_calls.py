"""Which ``Stage1Device`` calls the record views of mojo_simdjson_amd/document_stream.py make, without a GPU and without the
library: ``Window``, ``RowSelection``, ``ElementFields``, ``ListColumn`` and ``MapColumn`` over a stub device on CPU tensors.

The stub takes every call through the real method's signature (so that a positional and a keyword argument read the same),
writes down its name, its scalars and, for every tensor, which tensor it is a view of (by the storage's address), at which
byte, with which dtype, shape and strides -- a tensor nobody handed out is written down by its contents -- and answers with
outputs of the right shapes, a code-0 result and totals the test chooses (MSJ_CAPACITY while the room is below the total, as
the real calls do).  One window of 2 paths and 3 documents is made by hand; the other views come from it through the public
methods.  Pinned: the transcript of every public method; the first-guess room of the five column calls, clipped and not; the
grow-once second call; the blank record that stands in for zero rows; ValueError from a window without fields."""
import dataclasses
import inspect

import numpy as np
import pytest
import torch

from mojo_simdjson_amd import _lib, errors
from mojo_simdjson_amd import document_stream as ds
from mojo_simdjson_amd.device import Paths, Stage1Device

L, NT, D = 8192, 5000, 3    # the window's bytes, tokens and documents: the first guesses are below L and NT, not clipped
TOTAL = {"string_column": 5, "raw_column": 6, "array_column": 4, "array_elements": 7, "object_entries": 5, "dictionary": 2}
LAYOUT = {"string_column": ("total_bytes", "bytes_capacity", _lib.MsjStringColumnResult),
          "raw_column": ("total_bytes", "bytes_capacity", _lib.MsjRawColumnResult),
          "array_column": ("n_elements", "elements_capacity", _lib.MsjArrayColumnResult),
          "array_elements": ("n_elements", "elements_capacity", _lib.MsjArrayColumnResult),
          "object_entries": ("n_entries", "entries_capacity", _lib.MsjObjectEntriesResult)}
CALLS = list(LAYOUT) + ["select_elements", "dictionary", "compile_paths", "compile_predicates", "filter_rows", "take_rows", "cast_strings",
                        "aggregate"]


def word(n, n_paths=1):
    """A msj_select_documents_result that counts n records per column, as a tensor; its first word is the code, 0"""
    return torch.tensor(list(bytes(_lib.MsjSelectDocumentsResult(0, 0, int(n), int(n_paths), int(n), 0, 0))), dtype=torch.uint8)


def rows_of(d_select):
    return int(_lib.MsjSelectDocumentsResult.from_buffer_copy(bytes(d_select.tolist())).n_documents)


def ints(n, first=0):
    """n msj_field records, int64 numbers first, first + 1, ...; never an empty tensor"""
    out = torch.zeros((max(n, 1), 2), dtype=torch.int64)
    out[:, 0] = torch.arange(first, first + max(n, 1))
    out[:, 1] = ord("l") << 32
    return out


def letters(n):
    """n msj_field records, strings of one byte of the window each"""
    out = torch.zeros((max(n, 1), 2), dtype=torch.int64)
    out[:, 0] = torch.arange(max(n, 1)) % 26 | (1 << 32)
    out[:, 1] = ord('"') << 32
    return out


class Predicates:
    def __init__(self, dev):
        self.dev = dev

    def close(self):
        self.dev.calls.append(("close", {}))


class StubDevice:
    def __init__(self):
        self.calls, self.returns, self.sources, self._paths, self.totals, self.serial = [], [], [], [], dict(TOTAL), 0

    def register(self, name, t):
        self.sources.append((name, t))
        return t

    def describe(self, t, out=False):
        if isinstance(t, Paths):
            return ("paths", tuple(t.pointers))
        if not isinstance(t, torch.Tensor):
            return t
        if out:
            return ("out", str(t.dtype), tuple(t.shape))
        if t.numel() == 0:
            return ("empty", str(t.dtype), tuple(t.shape))
        at = t.data_ptr()
        for name, base in self.sources:
            lo = base.untyped_storage().data_ptr()
            if lo <= at < lo + base.untyped_storage().nbytes():
                return (name, at - lo, str(t.dtype), tuple(t.shape), tuple(t.stride()))
        return ("new", str(t.dtype), tuple(t.shape), t.flatten().tolist() if t.numel() <= 96 else None)

    def expected(self, name, **kw):
        """What ``calls`` holds for a call with the signature's defaults and kw"""
        sig = inspect.signature(getattr(Stage1Device, name))
        a = {k: p.default for k, p in sig.parameters.items() if k != "self"}
        assert not set(kw) - set(a) and not [k for k, v in a.items() if v is inspect.Parameter.empty and k not in kw], (name, kw)
        a.update(kw)
        return (name, {k: self.describe(v, name in LAYOUT and k in ("d_offsets", "d_valid")) for k, v in a.items()})

    def __getattr__(self, name):
        if name not in CALLS:
            raise AttributeError(name)
        sig = inspect.signature(getattr(Stage1Device, name))

        def call(*args, **kw):
            bound = sig.bind(self, *args, **kw)
            bound.apply_defaults()
            a = {k: v for k, v in bound.arguments.items() if k != "self"}
            self.calls.append((name, {k: self.describe(v, name in LAYOUT and k in ("d_offsets", "d_valid")) for k, v in a.items()}))
            out = getattr(self, "answer_" + name)(**a)
            self.serial += 1
            for j, t in enumerate(out if isinstance(out, tuple) else ()):
                if isinstance(t, torch.Tensor):
                    self.register(f"{name}#{self.serial}.{j}", t)
            self.returns.append(out)
            return out

        return call

    def layout(self, name, d_offsets, d_valid, capacity, room):
        total_field, _, result = LAYOUT[name]
        total = self.totals[name] if capacity else 0
        assert d_offsets.shape[0] >= capacity + 1 and d_valid.shape[0] >= max(capacity, 1)
        d_offsets[:capacity + 1] = torch.arange(capacity + 1) * total // max(capacity, 1)
        d_valid.fill_(1)
        return result(code=errors.CAPACITY if total > room else 0, n_rows=capacity, **{total_field: total}), total

    def answer_string_column(self, d_offsets, d_valid, capacity, bytes_capacity, **_):
        res, _ = self.layout("string_column", d_offsets, d_valid, capacity, bytes_capacity)
        return res, d_offsets, d_valid, torch.full((max(bytes_capacity, 1),), 97, dtype=torch.uint8)

    def answer_raw_column(self, d_offsets, d_valid, capacity, bytes_capacity, **_):
        res, _ = self.layout("raw_column", d_offsets, d_valid, capacity, bytes_capacity)
        return res, d_offsets, d_valid, torch.full((max(bytes_capacity, 1),), 49, dtype=torch.uint8)

    def answer_array_column(self, d_offsets, d_valid, capacity, elements_capacity, name="array_column", **_):
        res, total = self.layout(name, d_offsets, d_valid, capacity, elements_capacity)
        return res, d_offsets, d_valid, ints(elements_capacity, 100), word(total)

    def answer_array_elements(self, **a):
        return self.answer_array_column(name="array_elements", **a)

    def answer_object_entries(self, d_offsets, d_valid, capacity, entries_capacity, **_):
        res, total = self.layout("object_entries", d_offsets, d_valid, capacity, entries_capacity)
        return res, d_offsets, d_valid, letters(entries_capacity), ints(entries_capacity, 200), word(total), word(total)

    def answer_select_elements(self, paths, capacity, **_):
        fields = torch.stack([ints(capacity, 300 + 100 * p) for p in range(paths.n_paths)])
        return word(capacity, paths.n_paths), fields

    def answer_dictionary(self, rows, **_):
        nd = min(self.totals["dictionary"], rows)
        res = _lib.MsjDictionaryResult(code=0, n_rows=rows, n_values=rows, n_distinct=nd, dict_bytes=nd)
        codes = (torch.arange(max(rows, 1)) % max(nd, 1)).to(torch.int32)
        return (res, codes, torch.arange(nd + 1, dtype=torch.int64), torch.arange(max(nd, 1), dtype=torch.int32),
                torch.arange(97, 97 + max(nd, 1), dtype=torch.uint8))

    def answer_compile_paths(self, pointers):
        paths = Paths(None, 1, [p.encode() for p in pointers])
        self._paths.append(paths)
        return paths

    def answer_compile_predicates(self, specs, any):
        predicates = Predicates(self)
        self._paths.append(predicates)
        return predicates

    def answer_filter_rows(self, d_rows_select, d_list_offsets, **_):
        """Every other row passes"""
        rows = rows_of(d_rows_select)
        kept = torch.arange(0, rows, 2, dtype=torch.int32)
        d_keep, d_kept = torch.zeros(max(rows, 1), dtype=torch.uint8), torch.zeros(max(rows, 1), dtype=torch.int32)
        d_keep[kept.long()], d_kept[:kept.shape[0]] = 1, kept
        d_list = None if d_list_offsets is None else torch.searchsorted(kept.long(), d_list_offsets.contiguous())
        return _lib.MsjFilterRowsResult(code=0, n_rows=rows, n_kept=kept.shape[0]), d_keep, d_kept, word(kept.shape[0]), d_list

    def answer_take_rows(self, d_take, d_fields, out_capacity, **_):
        n, f = out_capacity, d_fields if d_fields.dim() == 3 else d_fields.unsqueeze(0)
        out = torch.zeros((f.shape[0], max(n, 1), 2), dtype=torch.int64)
        out[:, :n] = f[:, d_take[:n].long().clamp(0, f.shape[1] - 1)]
        return word(n), out, word(n, f.shape[0])

    def answer_cast_strings(self, d_rows, capacity, **_):
        """The records with 1000 added: a number record each"""
        out = ints(capacity)
        out[:capacity, 0] = d_rows[:capacity, 0] + 1000
        return word(capacity), out, word(capacity)

    def answer_aggregate(self, d_fields, d_rows_select, n_groups, groups_capacity, **_):
        n_columns = d_fields.shape[0] if d_fields.dim() == 3 else 1
        res = _lib.MsjAggregateResult(code=0, n_rows=rows_of(d_rows_select), n_groups=n_groups)
        return res, torch.zeros(n_columns * groups_capacity * 48, dtype=torch.uint8)


def make_window(dev, fields=True, **kw):
    """One window of D documents and the paths /a (the numbers 10 20 30) and /b (true false null), by hand"""
    reg = dev.register
    results = reg("results", torch.zeros(192, dtype=torch.uint8))
    results[144:192] = word(D, 2)
    idx = reg("d_idx", torch.arange(NT, dtype=torch.int32))
    d_fields = reg("d_fields", torch.stack([ints(D), ints(D)]))
    d_fields[0, :, 0] = torch.tensor([10, 20, 30])
    d_fields[1, :, 0] = 0
    d_fields[1, :, 1] = torch.tensor([ord(c) << 32 for c in "tfn"])
    tapes = np.zeros(D, dtype=ds.DOC_TAPE_DTYPE)
    tapes["code"] = 3
    selected = dict(d_fields=d_fields, paths=Paths(None, 1, [b"/a", b"/b"]), n_found=2 * D, d_select=results[144:192]) if fields else {}
    a = dict(base=4096, length=L, consumed=L, n_tokens=NT, n_documents=D, utf8_error=False, d_idx=idx,
             d_type=reg("d_type", torch.zeros(NT, dtype=torch.uint8)), d_depth=reg("d_depth", torch.zeros(NT, dtype=torch.int32)),
             d_doc_first=reg("d_doc_first", torch.tensor([0, 10, 20], dtype=torch.int32)),
             d_match=reg("d_match", torch.zeros(NT, dtype=torch.int32)), d_end=reg("d_end", idx + 1),
             d_flags=reg("d_flags", torch.zeros(NT, dtype=torch.uint8)),
             d_window=reg("d_window", (torch.arange(L) % 26 + 97).to(torch.uint8)), d_docs=results[32:64],
             d_numbers=reg("d_numbers", torch.zeros((11, 2), dtype=torch.int64)), d_numbers_result=results[64:96],
             d_tape=torch.zeros(2, dtype=torch.int64), d_string_buf=torch.zeros(16, dtype=torch.uint8),
             d_doc_tapes=torch.from_numpy(tapes.view("<i8").reshape(D, 4).copy()), dev=dev, **selected)
    a.update(kw)
    return ds.Window(**a)


class Expect:
    """The calls the views make, written from the issue's table: the window's own arrays filled in"""

    def __init__(self, dev, win):
        self.dev, self.w = dev, win

    def tokens(self, depth=True):
        w = self.w
        a = dict(d_idx=w.d_idx, n=w.n_tokens, d_type=w.d_type, d_match=w.d_match, d_end=w.d_end, d_flags=w.d_flags)
        return dict(a, d_depth=w.d_depth) if depth else a

    def numbers(self):
        w = self.w
        return dict(d_numbers=w.d_numbers, numbers_capacity=w.d_numbers.shape[0], d_numbers_result=w.d_numbers_result)

    def outs(self, rows):
        return dict(d_offsets=torch.empty(rows + 1, dtype=torch.int64), d_valid=torch.empty(max(rows, 1), dtype=torch.uint8), capacity=rows)

    def strings(self, fields, p, select, rows, room):
        return self.dev.expected("string_column", d_buf=self.w.d_window, length=self.w.length, d_fields=fields, p=p, d_select_result=select,
                                 bytes_capacity=room, **self.outs(rows))

    def raw(self, records, select, rows, room, compact):
        return self.dev.expected("raw_column", d_buf=self.w.d_window, length=self.w.length, d_rows=records, d_rows_select=select,
                                 bytes_capacity=room, compact=compact, **self.tokens(depth=False), **self.outs(rows))

    def array_column(self, fields, p, select, rows, room):
        return self.dev.expected("array_column", d_doc_first=self.w.d_doc_first, d_docs=self.w.d_docs, d_fields=fields, p=p,
                                 d_select_result=select, elements_capacity=room, **self.tokens(), **self.numbers(), **self.outs(rows))

    def array_elements(self, records, select, rows, room):
        return self.dev.expected("array_elements", d_rows=records, d_rows_select=select, elements_capacity=room, **self.tokens(),
                                 **self.numbers(), **self.outs(rows))

    def entries(self, records, select, rows, room):
        return self.dev.expected("object_entries", d_rows=records, d_rows_select=select, entries_capacity=room, **self.tokens(),
                                 **self.numbers(), **self.outs(rows))

    def dictionary(self, column, rows):
        """column: what the string call before it returned"""
        total = int(column[0].total_bytes)
        d_valid = column[2][:rows] if rows else torch.zeros(1, dtype=torch.uint8)
        return self.dev.expected("dictionary", d_offsets=column[1], d_bytes=column[3][:total], d_valid=d_valid, rows=rows)

    def cast(self, records, select, rows, kind, unit, keep_numbers):
        return self.dev.expected("cast_strings", d_window=self.w.d_window, length=self.w.length, d_rows=records, d_rows_select=select, kind=kind,
                                 unit=unit, keep_numbers=keep_numbers, capacity=rows, sync=False)

    def take(self, d_take, d_take_select, fields, select, n):
        return self.dev.expected("take_rows", d_take=d_take, d_take_select=d_take_select, d_fields=fields, d_rows_select=select, out_capacity=n,
                                 sync=False)

    def filter(self, specs, any, fields, select, rows, d_list_offsets=None):
        return [self.dev.expected("compile_predicates", specs=specs, any=any),
                self.dev.expected("filter_rows", predicates="predicates", d_buf=self.w.d_window, length=self.w.length, d_fields=fields,
                                  d_rows_select=select, capacity=rows, d_list_offsets=d_list_offsets), ("close", {})]

    def aggregate(self, fields, select, d_codes, n_groups):
        return self.dev.expected("aggregate", d_fields=fields, d_rows_select=select, d_codes=d_codes, n_groups=n_groups,
                                 groups_capacity=max(n_groups, 1))


def run(dev, fn, *args, **kw):
    """fn(...) with a fresh transcript; the predicates a filter compiled are no longer the device's to close"""
    dev.calls.clear(), dev.returns.clear()
    before = len(dev._paths)
    out = fn(*args, **kw)
    assert len(dev._paths) == before + sum(name == "compile_paths" for name, _ in dev.calls)   # the predicates are taken out again
    return out


@dataclasses.dataclass
class View:
    """What the test knows of one record view: the records as [n_columns, rows, 2], the select result that counts them, the
    column the methods below are asked for, and how the class spells its arguments"""
    obj: object
    fields: torch.Tensor
    select: torch.Tensor
    rows: int
    args: tuple           # () for a ListColumn, else the path
    p: int
    numbers: str          # "number_column" or "numbers"
    parent: object        # what elements() and entries() hand on
    documents: bool = False


@pytest.fixture()
def made():
    dev = StubDevice()
    win = make_window(dev)
    rows = dev.register("rows", torch.tensor([2, 0], dtype=torch.int32))
    sel = win.take(rows)
    col = win.elements("/a")
    ef = col.select(["/x", "/y"])
    mc = win.entries("/b")
    dev.calls.clear(), dev.returns.clear()
    return dev, win, sel, col, ef, mc, rows


def describe_predicates(dev):
    """Predicates objects in a transcript read as one word"""
    for _, a in dev.calls:
        if isinstance(a.get("predicates"), Predicates):
            a["predicates"] = "predicates"
    return dev.calls


def views(made):
    dev, win, sel, col, ef, mc, _ = made
    return {"window": View(win, win.d_fields, win.d_select, D, ("/b",), 1, "number_column", None, documents=True),
            "selection": View(sel, sel.fields, sel.d_select, 2, ("/a",), 0, "number_column", None),
            "element fields": View(ef, ef.fields, ef.d_select, 4, ("/y",), 1, "numbers", ef),
            "list column": View(col, col.fields.unsqueeze(0), col.d_select, 4, (), 0, "numbers", col)}


def empty_views(made):
    dev, win, _, _, _, _, _ = made
    sel = win.take(torch.zeros(0, dtype=torch.int32))
    dev.totals["array_column"] = 0
    col = win.elements("/a")
    dev.totals.update(TOTAL)
    ef = col.select(["/x", "/y"])
    assert sel.fields.shape == (2, 0, 2) and sel.n_rows == 0 and col.fields.shape == (0, 2) and col.n_elements == 0 and ef.fields.shape == (2, 0, 2)
    return {"selection": View(sel, sel.fields, sel.d_select, 0, ("/b",), 1, "number_column", None),
            "element fields": View(ef, ef.fields, ef.d_select, 0, ("/x",), 0, "numbers", ef),
            "list column": View(col, col.fields.unsqueeze(0), col.d_select, 0, (), 0, "numbers", col)}


def check_view(dev, win, v):
    """The methods every record view has, each once: its transcript and the shapes of what it returns.  rows == 0: the blank
    record stands in, capacity=0, columns of length 0."""
    e, rows, o = Expect(dev, win), v.rows, v.obj
    n_columns = v.fields.shape[0]
    fields = v.fields if rows else torch.zeros((n_columns, 1, 2), dtype=torch.int64)
    records = v.fields[v.p] if rows else torch.zeros((1, 2), dtype=torch.int64)
    length, n_tokens = win.length, win.n_tokens
    # the numbers: torch alone
    for dtype in (torch.int64, torch.float64):
        values, valid = run(dev, getattr(o, v.numbers), *v.args, dtype=dtype)
        assert dev.calls == [] and values.shape == valid.shape == (rows,) and values.dtype == dtype and valid.dtype == torch.bool
    with pytest.raises(ValueError):
        getattr(o, v.numbers)(*v.args, dtype=torch.int32)
    # the casts
    values, valid = run(dev, o.timestamps, *v.args, unit="ms")
    assert dev.calls == [e.cast(records, v.select, rows, "timestamp", "ms", False)]
    assert values.shape == valid.shape == (rows,) and values.dtype == torch.int64
    if rows:
        assert values.tolist() == (v.fields[v.p, :, 0] + 1000).tolist() and valid.all()
    values, valid = run(dev, o.parsed_numbers, *v.args)
    assert dev.calls == [e.cast(records, v.select, rows, "number", "ns", True)] and values.dtype == torch.float64
    values, valid = run(dev, o.parsed_numbers, *v.args, dtype=torch.int64, keep_numbers=False)
    assert dev.calls == [e.cast(records, v.select, rows, "number", "ns", False)] and values.dtype == torch.int64 and values.shape == (rows,)
    # the byte columns
    total = TOTAL["string_column"] if rows else 0
    offsets, data, valid = run(dev, o.strings, *v.args)
    assert dev.calls == [e.strings(fields, v.p, v.select, rows, min(length, 32 * rows + 4096))]
    assert offsets.shape == (rows + 1,) and data.shape == (total,) and valid.shape == (rows,) and valid.dtype == torch.bool
    run(dev, o.strings, *v.args, bytes_capacity=total + 1)
    assert dev.calls == [e.strings(fields, v.p, v.select, rows, total + 1)]
    cats = run(dev, o.categories, *v.args)
    assert dev.calls == [e.strings(fields, v.p, v.select, rows, min(length, 32 * rows + 4096)), e.dictionary(dev.returns[0], rows)]
    assert isinstance(cats, ds.DictionaryColumn) and cats.codes.shape == (rows,) and cats.n_distinct == min(2, rows)
    assert cats.valid.shape == (rows,) and cats.offsets.shape == (cats.n_distinct + 1,)
    total = TOTAL["raw_column"] if rows else 0
    for compact in (False, True):
        offsets, data, valid = run(dev, o.raw, *v.args, compact=compact)
        assert dev.calls == [e.raw(records, v.select, rows, min(length, 64 * rows + 4096), compact)]
        assert offsets.shape == (rows + 1,) and data.shape == (total,) and valid.shape == (rows,)
    run(dev, o.raw, *v.args, bytes_capacity=9)
    assert dev.calls == [e.raw(records, v.select, rows, 9, False)]
    # the nested columns
    room = min(n_tokens, 4 * rows + 4096)
    name = "array_column" if v.documents else "array_elements"
    total = TOTAL[name] if rows else 0
    inner = run(dev, o.elements, *v.args)
    assert dev.calls == [e.array_column(fields, v.p, v.select, rows, room) if v.documents else e.array_elements(records, v.select, rows, room)]
    assert isinstance(inner, ds.ListColumn) and inner.parent is v.parent and inner.window is win and inner.n_elements == total
    assert inner.offsets is dev.returns[0][1] and inner.d_select is dev.returns[0][4] and inner.valid.shape == (rows,)
    assert dev.describe(inner.fields) == dev.describe(dev.returns[0][3][:total])
    run(dev, o.elements, *v.args, elements_capacity=total + 2)
    assert dev.calls == [e.array_column(fields, v.p, v.select, rows, total + 2) if v.documents else
                         e.array_elements(records, v.select, rows, total + 2)]
    total = TOTAL["object_entries"] if rows else 0
    maps = run(dev, o.entries, *v.args)
    assert dev.calls == [e.entries(records, v.select, rows, room)]
    assert isinstance(maps, ds.MapColumn) and maps.parent is v.parent and maps.window is win and maps.n_entries == total
    assert maps.offsets is dev.returns[0][1] and maps.valid.shape == (rows,)
    assert maps.d_keys_select is dev.returns[0][5] and maps.d_values_select is dev.returns[0][6]
    assert dev.describe(maps.key_fields) == dev.describe(dev.returns[0][3][:total])
    assert dev.describe(maps.value_fields) == dev.describe(dev.returns[0][4][:total])
    run(dev, o.entries, *v.args, entries_capacity=total)
    assert dev.calls == [e.entries(records, v.select, rows, total)]


GROWN = [("strings", "string_column", "strings"), ("categories", "string_column", "strings"), ("raw", "raw_column", "raw"),
         ("elements", "array_elements", "array_elements"), ("entries", "object_entries", "entries")]


def check_grow_once(dev, win, v):
    """A total beyond the first guess: MSJ_CAPACITY, then one more call whose room is exactly that total, and no third"""
    e, rows = Expect(dev, win), v.rows
    records = v.fields[v.p]
    for method, call, expect in GROWN:
        if v.documents and method == "elements":
            call = "array_column"
        total = {"strings": 32 * rows + 4097, "categories": 32 * rows + 4099, "raw": 64 * rows + 4097}.get(method, 4 * rows + 4097)
        dev.totals[call] = total
        out = run(dev, getattr(v.obj, method), *v.args)
        dev.totals.update(TOTAL)
        one = {"string_column": lambda room: e.strings(v.fields, v.p, v.select, rows, room),
               "raw_column": lambda room: e.raw(records, v.select, rows, room, False),
               "array_column": lambda room: e.array_column(v.fields, v.p, v.select, rows, room),
               "array_elements": lambda room: e.array_elements(records, v.select, rows, room),
               "object_entries": lambda room: e.entries(records, v.select, rows, room)}[call]
        assert dev.calls[:2] == [one(total - 1 if method != "categories" else total - 3), one(total)], (method, dev.calls)
        assert [name for name, _ in dev.calls[2:]] == (["dictionary"] if method == "categories" else [])
        assert dev.returns[0][0].code == errors.CAPACITY and dev.returns[1][0].code == 0
        if method in ("strings", "raw"):
            assert out[1].shape == (total,)
        elif method == "elements":
            assert out.n_elements == total
        elif method == "entries":
            assert out.n_entries == total


@pytest.mark.parametrize("name", ["window", "selection", "element fields", "list column"])
def test_every_view_makes_the_same_calls(made, name):
    dev, win = made[:2]
    check_view(dev, win, views(made)[name])


@pytest.mark.parametrize("name", ["window", "selection", "element fields", "list column"])
def test_grow_once(made, name):
    dev, win = made[:2]
    check_grow_once(dev, win, views(made)[name])
    # a code that is not MSJ_CAPACITY, or a second MSJ_CAPACITY, is the stream's error
    v = views(made)[name]
    dev.answer_string_column = lambda d_offsets, d_valid, capacity, **_: (
        _lib.MsjStringColumnResult(code=errors.CAPACITY, n_rows=capacity, total_bytes=1 << 40), d_offsets, d_valid, torch.zeros(1, dtype=torch.uint8))
    with pytest.raises(ds.DocumentStreamError) as err:
        run(dev, v.obj.strings, *v.args)
    assert err.value.code == errors.CAPACITY and [n for n, _ in dev.calls] == ["string_column"] * 2 and str(err.value).startswith("window at 4096:")


def test_first_guesses_are_clipped(made):
    """A window shorter than the guess: the room is the window's bytes, or its tokens"""
    dev, win = made[:2]
    small = dataclasses.replace(win, length=64, n_tokens=40)
    e = Expect(dev, small)
    run(dev, small.strings, "/a")
    assert dev.calls == [e.strings(win.d_fields, 0, win.d_select, D, 64)]
    run(dev, small.raw, "/a")
    assert dev.calls == [e.raw(win.d_fields[0], win.d_select, D, 64, False)]
    run(dev, small.elements, "/a")
    assert dev.calls == [e.array_column(win.d_fields, 0, win.d_select, D, 40)]
    col = run(dev, small.entries, "/a").values()
    assert dev.calls == [e.entries(win.d_fields[0], win.d_select, D, 40)]
    run(dev, col.elements)
    assert dev.calls == [e.array_elements(col.fields, col.d_select, 5, 40)]
    run(dev, col.strings)
    assert dev.calls == [e.strings(col.fields.unsqueeze(0), 0, col.d_select, 5, 64)]


@pytest.mark.parametrize("name", ["selection", "element fields", "list column"])
def test_zero_rows(made, name):
    dev, win = made[:2]
    check_view(dev, win, empty_views(made)[name])


def test_zero_rows_of_the_particular_methods(made):
    """take of no row, and select, where and stats over no element: a blank record, capacity 0"""
    dev, win = made[:2]
    e = Expect(dev, win)
    blank, blanks = torch.zeros((1, 2), dtype=torch.int64), torch.zeros((2, 1, 2), dtype=torch.int64)
    none = torch.zeros(0, dtype=torch.int32)
    sel = run(dev, win.take, none)
    assert dev.calls == [e.take(torch.zeros(1, dtype=torch.int32), word(0), win.d_fields, win.d_select, 0)]
    assert sel.fields.shape == (2, 0, 2) and sel.rows.shape == (0,) and sel.column("/a").shape == (0,) and sel.values("/a") == []
    stats = run(dev, sel.stats, ["/a", "/b"])
    assert dev.calls == [e.aggregate(blanks, sel.d_select, None, 1)] and stats.n_groups == 1 and stats.n_values.tolist() == [[0], [0]]
    stats = run(dev, sel.stats, ["/a"], by="/b", cast={"/a": "number"})
    assert dev.calls == [e.strings(blanks, 1, sel.d_select, 0, 4096), e.dictionary(dev.returns[0], 0),
                         e.aggregate(blank.unsqueeze(0), sel.d_select, torch.zeros(1, dtype=torch.int32), 0)]
    assert stats.n_groups == 0 and stats.records.shape == (1, 0, 48)
    views_ = empty_views(made)
    col, ef = views_["list column"].obj, views_["element fields"].obj
    got = run(dev, col.select, ["/x", "/y"])
    assert dev.calls == [dev.expected("compile_paths", pointers=["/x", "/y"]),
                         dev.expected("select_elements", paths=dev.returns[0], d_buf=win.d_window, length=L, d_rows=blank, d_rows_select=col.d_select,
                                      capacity=0, sync=False, **e.tokens(), **e.numbers())]
    assert got.fields.shape == (2, 0, 2) and got.to_python() == [[], [], []] and col.to_python() == [[], [], []]
    kept = run(dev, col.where, [(0, ">", 1)])
    assert describe_predicates(dev) == e.filter([(0, ">", 1)], False, blank.unsqueeze(0), col.d_select, 0, col.offsets) + \
        [e.take(none, dev.returns[1][3], blank.unsqueeze(0), col.d_select, 0)]
    assert kept.n_elements == 0 and kept.offsets.tolist() == [0] * 4
    kept = run(dev, ef.where, [("/x", ">", 1)])
    assert describe_predicates(dev) == e.filter([(0, ">", 1)], False, blanks, ef.d_select, 0, col.offsets) + \
        [e.take(none, dev.returns[1][3], blank.unsqueeze(0), col.d_select, 0), e.take(none, dev.returns[1][3], blanks, ef.d_select, 0)]
    assert kept.n_elements == 0 and kept.list_column.n_elements == 0
    for per_row, groups in ((False, 1), (True, D)):
        run(dev, col.stats, per_row=per_row)
        assert dev.calls == [e.aggregate(blank.unsqueeze(0), col.d_select, torch.zeros(1, dtype=torch.int32) if per_row else None, groups)]
        run(dev, ef.stats, ["/y"], per_row=per_row)
        assert dev.calls == [e.aggregate(blank.unsqueeze(0), ef.d_select, torch.zeros(1, dtype=torch.int32) if per_row else None, groups)]


def test_window(made):
    """What only a Window has: the host copies, cast, take, where, stats, the documents"""
    dev, win, sel, _, _, _, rows = made
    e, F, S = Expect(dev, win), win.d_fields, win.d_select
    assert run(dev, win.column, "/a")["bits"].tolist() == [10, 20, 30] and run(dev, win.column, 1)["type"].tolist() == [ord(c) for c in "tfn"]
    assert run(dev, win.values, "/a") == [10, 20, 30] and run(dev, win.values, "/b") == [True, False, None] and dev.calls == []
    assert run(dev, win.number_column, "/a", torch.int64)[0].tolist() == [10, 20, 30] and dev.calls == []
    records, d_select = run(dev, win.cast, "/a", "timestamp", "us", keep_numbers=True)
    assert dev.calls == [e.cast(F[0], S, D, "timestamp", "us", True)] and records.shape == (D, 2) and d_select is dev.returns[0][2]
    assert dev.describe(records) == dev.describe(dev.returns[0][1][:D])
    # take: made in the fixture
    got = run(dev, win.take, rows)
    assert dev.calls == [e.take(rows, word(2), F, S, 2)] and isinstance(got, ds.RowSelection)
    assert got.keep is None and got.rows is rows and got.window is win and got.paths is win.paths and got.n_rows == 2
    assert got.d_select is dev.returns[0][2] and dev.describe(got.fields) == dev.describe(dev.returns[0][1][:, :2])
    assert got.values("/a") == [30, 10] and got.values("/b") == [None, True] and got.column(0)["bits"].tolist() == [30, 10]
    # where: the filter, then the take of the original records
    got = run(dev, win.where, [("/a", ">", 15), ("not", (1, "found"))], any=True)
    kept, kept_select = dev.returns[1][2], dev.returns[1][3]
    assert describe_predicates(dev) == e.filter([(0, ">", 15), ("not", (1, "found"))], True, F, S, D) + [e.take(kept[:2], kept_select, F, S, 2)]
    assert got.keep.tolist() == [True, False, True] and got.rows.tolist() == [0, 2] and got.values("/a") == [10, 30]
    assert got.d_select is dev.returns[2][2]
    # ... with a cast: the predicates see a copy whose cast columns are cast, re-numbered; the take sees the originals
    got = run(dev, win.where, [("/b", "found"), ("/a", "<", 1015)], cast={"/a": "number"})
    seen = torch.stack([ints(D), F[1]])
    seen[0, :, 0] = F[0, :, 0] + 1000
    kept, kept_select = dev.returns[2][2], dev.returns[2][3]
    assert describe_predicates(dev) == [e.cast(F[0], S, D, "number", "ns", True)] + \
        e.filter([(1, "found"), (0, "<", 1015)], False, seen, S, D) + [e.take(kept[:2], kept_select, F, S, 2)]
    assert got.values("/a") == [10, 30]
    # stats: one group; by a path; cast first
    stats = run(dev, win.stats, ["/b", "/a"])
    assert dev.calls == [e.aggregate(torch.stack([F[1], F[0]]), S, None, 1)]
    assert isinstance(stats, ds.GroupStats) and stats.pointers == ["/b", "/a"] and stats.keys is None and stats.records.shape == (2, 1, 48)
    stats = run(dev, win.stats, ["/a"], by="/b", cast={"/a": ("timestamp", "s")})
    assert dev.calls == [e.strings(F, 1, S, D, 32 * D + 4096), e.dictionary(dev.returns[0], D), e.cast(F[0], S, D, "timestamp", "s", False),
                         e.aggregate(seen[:1], S, dev.returns[1][1][:D], 2)]
    assert stats.keys.n_distinct == 2 and stats.n_groups == 2 and stats.to_python()[0]["key"] == "a"
    with pytest.raises(ValueError):
        win.stats([])
    # the documents: host copies, no call
    assert run(dev, win.documents) == [None] * D and run(dev, win.document, 1) is None and dev.calls == []
    assert run(dev, win.document_offsets) == [4096, 4106, 4116] and dev.calls == []


def test_row_selection(made):
    dev, win, sel, _, _, _, rows = made
    e = Expect(dev, win)
    assert sel.n_rows == 2 and sel.rows is rows and sel.keep is None
    assert run(dev, sel.column, "/a")["bits"].tolist() == [30, 10] and run(dev, sel.values, "/b") == [None, True] and dev.calls == []
    run(dev, sel.stats, ["/a"])
    assert dev.calls == [e.aggregate(sel.fields[:1].clone(), sel.d_select, None, 1)]
    run(dev, sel.stats, ["/a"], by="/b", cast={"/a": "number"})
    cast = ints(2)
    cast[:, 0] = torch.tensor([1030, 1010])
    assert dev.calls == [e.strings(sel.fields, 1, sel.d_select, 2, 32 * 2 + 4096), e.dictionary(dev.returns[0], 2),
                         e.cast(sel.fields[0], sel.d_select, 2, "number", "ns", True), e.aggregate(cast.unsqueeze(0), sel.d_select, dev.returns[1][1][:2], 2)]


def test_list_column(made):
    """What only a ListColumn has: select, where, stats, to_python"""
    dev, win, _, col, _, _, _ = made
    e = Expect(dev, win)
    assert col.n_elements == 4 and col.parent is None and col.offsets.tolist() == [0, 1, 2, 4]
    assert run(dev, col.to_python) == [[100], [101], [102, 103]] and dev.calls == []
    ef = run(dev, col.select, ["/x", "/y"])
    assert dev.calls == [dev.expected("compile_paths", pointers=["/x", "/y"]),
                         dev.expected("select_elements", paths=dev.returns[0], d_buf=win.d_window, length=L, d_rows=col.fields,
                                      d_rows_select=col.d_select, capacity=4, sync=False, **e.tokens(), **e.numbers())]
    assert isinstance(ef, ds.ElementFields) and ef.list_column is col and ef.paths is dev.returns[0] and ef.d_select is dev.returns[1][0]
    assert dev.describe(ef.fields) == dev.describe(dev.returns[1][1][:, :4]) and ef.n_elements == 4
    again = run(dev, col.select, ef.paths)   # compiled paths are taken as they are
    assert [name for name, _ in dev.calls] == ["select_elements"] and again.paths is ef.paths
    kept = run(dev, col.where, [(0, ">", 1)], any=True)
    assert describe_predicates(dev) == e.filter([(0, ">", 1)], True, col.fields.unsqueeze(0), col.d_select, 4, col.offsets) + \
        [e.take(dev.returns[1][2][:2], dev.returns[1][3], col.fields.unsqueeze(0), col.d_select, 2)]
    assert isinstance(kept, ds.ListColumn) and kept.to_python() == [[100], [], [102]] and kept.valid is col.valid and kept.parent is col.parent
    assert kept.d_select is dev.returns[2][2] and kept.offsets is dev.returns[1][4]
    cast = ints(4, 1100)
    kept = run(dev, col.where, [(0, ">", 1)], cast={0: ("timestamp", "ms")})
    assert describe_predicates(dev) == [e.cast(col.fields, col.d_select, 4, "timestamp", "ms", False)] + \
        e.filter([(0, ">", 1)], False, cast.unsqueeze(0), col.d_select, 4, col.offsets) + \
        [e.take(dev.returns[2][2][:2], dev.returns[2][3], col.fields.unsqueeze(0), col.d_select, 2)]
    assert kept.to_python() == [[100], [], [102]]
    with pytest.raises(IndexError):
        col.where([(1, "found")])
    stats = run(dev, col.stats)
    assert dev.calls == [e.aggregate(col.fields.unsqueeze(0).clone(), col.d_select, None, 1)] and stats.pointers == [""] and stats.keys is None
    stats = run(dev, col.stats, per_row=True, cast="number")
    assert dev.calls == [e.cast(col.fields, col.d_select, 4, "number", "ns", True),
                         e.aggregate(cast.unsqueeze(0), col.d_select, torch.tensor([0, 1, 2, 2], dtype=torch.int32), D)]
    assert stats.n_groups == D


def test_element_fields(made):
    """What only an ElementFields has: the host copies, stats per row, where with the list column rebuilt, to_python"""
    dev, win, _, col, ef, _, _ = made
    e = Expect(dev, win)
    assert run(dev, ef.column, "/y")["bits"].tolist() == [400, 401, 402, 403] and run(dev, ef.values, "/x") == [300, 301, 302, 303]
    assert run(dev, ef.to_python) == [[{"/x": 300, "/y": 400}], [{"/x": 301, "/y": 401}], [{"/x": 302, "/y": 402}, {"/x": 303, "/y": 403}]]
    assert dev.calls == []
    stats = run(dev, ef.stats, ["/y", "/x"])
    assert dev.calls == [e.aggregate(torch.stack([ef.fields[1], ef.fields[0]]), ef.d_select, None, 1)] and stats.pointers == ["/y", "/x"]
    run(dev, ef.stats, ["/x"], per_row=True)
    assert dev.calls == [e.aggregate(ef.fields[:1].clone(), ef.d_select, torch.tensor([0, 1, 2, 2], dtype=torch.int32), D)]
    stats = run(dev, ef.stats, ["/x"], by="/y", cast={"/x": "number"})
    assert dev.calls == [e.strings(ef.fields, 1, ef.d_select, 4, 32 * 4 + 4096), e.dictionary(dev.returns[0], 4),
                         e.cast(ef.fields[0], ef.d_select, 4, "number", "ns", True),
                         e.aggregate(ints(4, 1300).unsqueeze(0), ef.d_select, dev.returns[1][1][:4], 2)]
    assert stats.keys.n_distinct == 2
    with pytest.raises(ValueError):
        ef.stats(["/x"], by="/y", per_row=True)
    kept = run(dev, ef.where, [("/y", ">", 1)])
    d_kept, d_kept_select = dev.returns[1][2][:2], dev.returns[1][3]
    assert describe_predicates(dev) == e.filter([(1, ">", 1)], False, ef.fields, ef.d_select, 4, col.offsets) + \
        [e.take(d_kept, d_kept_select, col.fields.unsqueeze(0), col.d_select, 2), e.take(d_kept, d_kept_select, ef.fields, ef.d_select, 2)]
    assert isinstance(kept, ds.ElementFields) and kept.paths is ef.paths and kept.values("/x") == [300, 302] and kept.n_elements == 2
    assert kept.list_column.to_python() == [[100], [], [102]] and kept.list_column.parent is col.parent and kept.d_select is dev.returns[3][2]
    kept = run(dev, ef.where, [("/y", ">", 1)], cast={"/y": "number"})
    assert describe_predicates(dev)[0] == e.cast(ef.fields[1], ef.d_select, 4, "number", "ns", True)
    assert describe_predicates(dev)[1:4] == e.filter([(0, ">", 1)], False, ints(4, 1400).unsqueeze(0), ef.d_select, 4, col.offsets)
    assert [name for name, _ in dev.calls[4:]] == ["take_rows", "take_rows"] and kept.values("/y") == [400, 402]


def test_map_column(made):
    dev, win, _, _, _, mc, _ = made
    e = Expect(dev, win)
    assert mc.n_entries == 5 and mc.parent is None and mc.offsets.tolist() == [0, 1, 3, 5]
    keys = mc.key_fields.unsqueeze(0)
    offsets, data, valid = run(dev, mc.keys)
    assert dev.calls == [e.strings(keys, 0, mc.d_keys_select, 5, 32 * 5 + 4096)] and offsets.shape == (6,) and valid.shape == (5,)
    run(dev, mc.keys, bytes_capacity=11)
    assert dev.calls == [e.strings(keys, 0, mc.d_keys_select, 5, 11)]
    cats = run(dev, mc.key_categories)
    assert dev.calls == [e.strings(keys, 0, mc.d_keys_select, 5, 32 * 5 + 4096), e.dictionary(dev.returns[0], 5)] and cats.codes.shape == (5,)
    run(dev, mc.key_categories, bytes_capacity=12)
    assert dev.calls[0] == e.strings(keys, 0, mc.d_keys_select, 5, 12)
    dev.totals["string_column"] = 32 * 5 + 4097
    run(dev, mc.keys)
    dev.totals.update(TOTAL)
    assert dev.calls == [e.strings(keys, 0, mc.d_keys_select, 5, 32 * 5 + 4096), e.strings(keys, 0, mc.d_keys_select, 5, 32 * 5 + 4097)]
    schema = run(dev, mc.schema)
    assert [name for name, _ in dev.calls] == ["string_column", "dictionary"] and schema == [("a", 3, {"l"}), ("b", 2, {"l"})]
    values = run(dev, mc.values)
    assert dev.calls == [] and isinstance(values, ds.ListColumn) and values.parent is mc and values.window is win
    assert values.offsets is mc.offsets and values.valid is mc.valid and values.fields is mc.value_fields and values.d_select is mc.d_values_select
    assert run(dev, mc.to_python) == [{"a": 200}, {"b": 201, "c": 202}, {"d": 203, "e": 204}] and dev.calls == []
    # the values are a list column like any other: a map of maps
    inner = run(dev, values.entries)
    assert dev.calls == [e.entries(mc.value_fields, mc.d_values_select, 5, 4 * 5 + 4096)] and inner.parent is values
    raw = run(dev, values.raw)
    assert dev.calls == [e.raw(mc.value_fields, mc.d_values_select, 5, 64 * 5 + 4096, False)]


RECORD_METHODS = [("column", ("/a",)), ("values", ("/a",)), ("number_column", ("/a",)), ("strings", ("/a",)), ("categories", ("/a",)),
                  ("raw", ("/a",)), ("elements", ("/a",)), ("entries", ("/a",)), ("cast", ("/a", "number")), ("timestamps", ("/a",)),
                  ("parsed_numbers", ("/a",)), ("where", ([("/a", "found")],)), ("stats", (["/a"],)),
                  ("take", (torch.zeros(1, dtype=torch.int32),))]


def test_window_without_fields():
    dev = StubDevice()
    win = make_window(dev, fields=False)
    for method, args in RECORD_METHODS:
        with pytest.raises(ValueError, match="select="):
            getattr(win, method)(*args)
    assert dev.calls == [] and win.documents() == [None] * D
